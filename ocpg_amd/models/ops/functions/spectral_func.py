"""Autograd binding of csrc/spectral.hip: the LFM block's spectral gate as one pass each way; of csrc/lfm_dft.hip and
csrc/lfm_dft_any.hip: both Fourier transforms on the channels-last map, and the plan of every line length up to 256; of
csrc/lfm_dft_czt.hip: the same with a chirp-z line transform on one or both axes."""
import functools
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import DTYPE_CODE as _DT, check, lib


class SpectralGate(Function):
    @staticmethod
    def forward(ctx, spec, coef, high):
        """spec complex64 [N,C,h,w], coef [N], high [h,w] (no gradient) -> fp32 [N,2C,h,w] = cat(Re, Im)(spec * (1 - coef*high))."""
        spec = spec.contiguous()
        coef, high = coef.float().contiguous(), high.float().contiguous()
        n, c, h, w = spec.shape
        out = torch.empty((n, 2 * c, h, w), dtype=torch.float32, device=spec.device)
        check(lib().ocpg_spectral_gate_fwd(torch.view_as_real(spec).data_ptr(), coef.data_ptr(), high.data_ptr(), n, c, h * w, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "ocpg_spectral_gate_fwd")
        ctx.save_for_backward(spec, coef, high)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        spec, coef, high = ctx.saved_tensors
        n, c, h, w = spec.shape
        gout = gout.float().contiguous()
        dx = torch.empty((n, c, h, w, 2), dtype=torch.float32, device=spec.device)
        part = torch.empty((n, c * ((h * w + 255) // 256)), dtype=torch.float32, device=spec.device)
        check(lib().ocpg_spectral_gate_bwd(gout.data_ptr(), torch.view_as_real(spec).data_ptr(), coef.data_ptr(), high.data_ptr(), n, c, h * w,
                                           dx.data_ptr(), part.data_ptr(), torch.cuda.current_stream().cuda_stream), "ocpg_spectral_gate_bwd")
        return torch.view_as_complex(dx), part.sum(1), None


def spectral_gate(spec, coef, high):
    return SpectralGate.apply(spec, coef, high)


class WindowMeans3x3(Function):
    """x [N,C,h,w] fp32 -> [N, C*9]: mean of every plane over the nine (h-2)x(w-2) windows at offsets (ky,kx) (csrc/lfm.hip)."""

    @staticmethod
    def forward(ctx, x, as_bf16):
        x = x.contiguous()
        n, c, h, w = x.shape
        out = torch.empty((n, c * 9), dtype=torch.float32, device=x.device)
        check(lib().ocpg_window_means3x3_fwd(x.data_ptr(), n * c, h, w, int(as_bf16), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "ocpg_window_means3x3_fwd")
        ctx.shape = (n, c, h, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gm):
        n, c, h, w = ctx.shape
        gm = gm.float().contiguous()
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=gm.device)
        check(lib().ocpg_window_means3x3_bwd(gm.data_ptr(), n * c, h, w, dx.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "ocpg_window_means3x3_bwd")
        return dx, None


class WindowMeans3x3CL(Function):
    """WindowMeans3x3 for x [N,C,h,w] fp32 in CHANNELS-LAST memory (round 4), same result [N, C*9]."""

    @staticmethod
    def forward(ctx, x, as_bf16):
        xs = x.permute(0, 2, 3, 1)
        assert xs.is_contiguous() and xs.dtype == torch.float32
        n, h, w, c = xs.shape
        bands = int(lib().ocpg_window_sums3x3_cl_bands(h))
        part = torch.empty((n, bands, c * 9), dtype=torch.float32, device=x.device)
        check(lib().ocpg_window_sums3x3_cl(xs.data_ptr(), n, h, w, c, int(as_bf16), part.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "ocpg_window_sums3x3_cl")
        ctx.shape = (n, c, h, w)
        return part.sum(1) * (1.0 / ((h - 2) * (w - 2)))

    @staticmethod
    @once_differentiable
    def backward(ctx, gm):
        n, c, h, w = ctx.shape
        gm = gm.float().contiguous()
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=gm.device)
        check(lib().ocpg_window_means3x3_bwd_cl(gm.data_ptr(), n, h, w, c, None, dx.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "ocpg_window_means3x3_bwd_cl")
        return dx.permute(0, 3, 1, 2), None


def conv3x3_valid_spatial_mean(x, weight, bias, as_bf16):
    """== F.conv2d(x, weight, bias).mean(dim=(2, 3)) for a 3x3 valid convolution, without the convolution.  `weight` is the copy
    the convolution would have used (bf16 under autocast): the products are the same, only the summation order differs."""
    cl = x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] > 1 and x.permute(0, 2, 3, 1).is_contiguous() and x.shape[0] <= 65535
    m = WindowMeans3x3CL.apply(x, as_bf16) if cl else WindowMeans3x3.apply(x, as_bf16)
    with torch.autocast(device_type=x.device.type, enabled=False):
        return torch.nn.functional.linear(m, weight.float().flatten(1), None if bias is None else bias.float())


class SpectralGateCL(Function):
    """The gate with its [Re || Im] side in CHANNELS-LAST memory and the 1x1 convs' compute dtype (csrc/spectral.hip c2p / p2c):
    the result is a [N, 2C, h, w] tensor whose memory is [N, h, w, 2C], so the following 1x1 convs are plain GEMMs on it and no
    cast / layout copy sits between the FFT and the GEMM."""

    @staticmethod
    def forward(ctx, spec, coef, high, dtype):
        spec = spec.contiguous()
        coef, high = coef.float().contiguous(), high.float().contiguous()
        n, c, h, w = spec.shape
        pair = torch.empty((n, h, w, 2 * c), dtype=dtype, device=spec.device)
        check(lib().ocpg_spectral_c2p(torch.view_as_real(spec).data_ptr(), coef.data_ptr(), high.data_ptr(), n, c, h * w, pair.data_ptr(),
                                      _DT[dtype], torch.cuda.current_stream().cuda_stream), "ocpg_spectral_c2p")
        ctx.save_for_backward(spec, coef, high)
        return pair.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        spec, coef, high = ctx.saved_tensors
        n, c, h, w = spec.shape
        g = gz.permute(0, 2, 3, 1).contiguous()
        if g.dtype not in _DT:
            g = g.float()
        dx = torch.empty((n, c, h, w, 2), dtype=torch.float32, device=spec.device)
        nb = ((c + 63) // 64) * ((h * w + 63) // 64)
        part = torch.empty((n, nb), dtype=torch.float32, device=spec.device)
        check(lib().ocpg_spectral_p2c(g.data_ptr(), torch.view_as_real(spec).data_ptr(), coef.data_ptr(), high.data_ptr(), n, c, h * w,
                                      dx.data_ptr(), part.data_ptr(), _DT[g.dtype], torch.cuda.current_stream().cuda_stream), "ocpg_spectral_p2c")
        return torch.view_as_complex(dx), part.sum(1), None, None


class PairToComplex(Function):
    """y [N, 2C, h, w] in channels-last memory (any of fp32 / bf16 / fp16) -> complex64 [N, C, h, w] = y[:, :C] + i y[:, C:]
    (`torch.complex(*torch.chunk(y.float(), 2, dim=1))`, models/modules.py:52-53) in one transposing pass each way."""

    @staticmethod
    def forward(ctx, y):
        n, c2, h, w = y.shape
        src = y.permute(0, 2, 3, 1).contiguous()
        if src.dtype not in _DT:
            src = src.float()
        out = torch.empty((n, c2 // 2, h, w, 2), dtype=torch.float32, device=y.device)
        check(lib().ocpg_spectral_p2c(src.data_ptr(), None, None, None, n, c2 // 2, h * w, out.data_ptr(), None, _DT[src.dtype],
                                      torch.cuda.current_stream().cuda_stream), "ocpg_spectral_p2c")
        ctx.dtype = y.dtype
        return torch.view_as_complex(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gc):
        gc = gc.contiguous()
        n, c, h, w = gc.shape
        dt = ctx.dtype if ctx.dtype in _DT else torch.float32
        pair = torch.empty((n, h, w, 2 * c), dtype=dt, device=gc.device)
        check(lib().ocpg_spectral_c2p(torch.view_as_real(gc).data_ptr(), None, None, n, c, h * w, pair.data_ptr(), _DT[dt],
                                      torch.cuda.current_stream().cuda_stream), "ocpg_spectral_c2p")
        return pair.permute(0, 3, 1, 2).to(ctx.dtype)


def spectral_gate_cl(spec, coef, high, dtype):
    return SpectralGateCL.apply(spec, coef, high, dtype)


def pair_to_complex(y):
    return PairToComplex.apply(y)


class IFFT2Real(Function):
    """ifft2(z, s=(h, w)).real of a complex spectrum (models/modules.py:53-54) as one node.  autograd's backward of `.real` first builds
    a complex tensor (zeros + strided copy of the gradient: two passes over a [2560, 48, 80] complex map at the finest level) and runs
    a complex-to-complex transform on it; the gradient is REAL, so the same result is the real-to-complex transform
    fft2(g, norm="forward") -- half the butterflies and no complex staging."""

    @staticmethod
    def forward(ctx, z, h, w):
        ctx.sizes = (tuple(z.shape[-2:]), (h, w))
        return torch.fft.ifft2(z, s=(h, w)).real

    @staticmethod
    def backward(ctx, g):
        (zh, zw), (h, w) = ctx.sizes
        gz = torch.fft.fft2(g if g.dtype == torch.float32 else g.float(), norm="forward")
        if (zh, zw) != (h, w):          # ifft2 cropped / zero-padded its input to s: the mirror image on the way back
            gz = torch.nn.functional.pad(gz[..., :min(zh, h), :min(zw, w)], (0, max(zw - w, 0), 0, max(zh - h, 0)))
        return gz, None, None


def ifft2_real(z, h, w):
    return IFFT2Real.apply(z, int(h), int(w))


# ---- the transforms themselves on channels-last maps (csrc/lfm_dft.hip) ---------------------------------------------------------
def dft_supported(h, w):
    return bool(lib().ocpg_lfm_dft_supported(int(h), int(w)))


def _twiddles(n, device):
    """The tables of a line transform of length n (include/ocpg_hip.h): exp(-2 pi i m / n), then the L1- and the L2-point DFT matrices,
    formed in fp64: float2 [n + L1^2 + L2^2]"""
    from ....util.misc import memo

    def make():
        code = int(lib().ocpg_lfm_dft_split(int(n)))
        assert code, f"length {n} is not served by csrc/lfm_dft.hip"
        l1, l2 = code >> 8, code & 255

        def angles(idx, m):
            a = idx.to(torch.float64) * (-2.0 * torch.pi / m)
            return torch.stack([a.cos(), a.sin()], -1)
        parts = [angles(torch.arange(n), n)]
        for r in (l1, l2):
            k = torch.arange(r)
            parts.append(angles((k[:, None] * k[None, :]).remainder(r).flatten(), r))
        return torch.cat(parts).float().contiguous().to(device)
    return memo("lfm_tw", n, device, make)


# ---- every length 1..256 (csrc/lfm_dft_any.hip) -------------------------------------------------------------------------------
MAX_ANY = 256          # the longest line csrc/lfm_dft_any.hip serves
_MAXR = 16             # the largest stage held in registers


def _smooth_plans(n):
    """Every way to write n as a product of at most three stages in 2.._MAXR, ascending within a plan."""
    out = []
    for a in range(2, _MAXR + 1):
        if n == a:
            out.append((a,))
        if n % a:
            continue
        for b in range(a, _MAXR + 1):
            if n // a == b:
                out.append((a, b))
            if (n // a) % b:
                continue
            c = n // a // b
            if b <= c <= _MAXR:
                out.append((a, b, c))
    return out


@functools.lru_cache(maxsize=None)
def dft_plan(n):
    """The stages (r1, r2, r3) of the line transform of length n in csrc/lfm_dft_any.hip, product n, for 1 <= n <= 256; None otherwise.
    The rule: if n is a product of at most three stages <= 16, the plan with the FEWEST stages, among those the SMALLEST SUM of stages,
    among those the smallest first stage (then second); stages ascending, unused stages are 1 and stand in front: 125 = (5, 5, 5),
    250 = (5, 5, 10), 256 = (1, 16, 16), 13 = (1, 1, 13).  Any other n <= 256 is m * p with ONE prime 17 <= p <= 251 and m <= 15:
    (1, m, p), the direct length-p stage last (where the passes along w can use the half spectrum and real outputs)."""
    n = int(n)
    if n < 1 or n > MAX_ANY:
        return None
    if n == 1:
        return (1, 1, 1)
    plans = _smooth_plans(n)
    if plans:
        best = min(plans, key=lambda p: (len(p), sum(p), p))
        return (1,) * (3 - len(best)) + best
    p = max(f for f in range(2, n + 1) if n % f == 0 and all(f % d for d in range(2, int(f ** 0.5) + 1)))
    m = n // p
    assert p > _MAXR and m < _MAXR, (n, p, m)       # holds for every n <= 256 (tests/test_lfm_dft_any_cpu.py walks them)
    return (1, m, p)


@functools.lru_cache(maxsize=None)
def _axis_plan(n):
    """The plan the _any entry points get for an axis: the old L1 x L2 split where csrc/lfm_dft.hip serves the length, else dft_plan."""
    code = int(lib().ocpg_lfm_dft_split(int(n)))
    return (code >> 8, code & 255, 1) if code else dft_plan(n)


def dft_any_supported(h, w):
    return dft_plan(h) is not None and dft_plan(w) is not None


def _twiddles_any(n, device):
    """The table of a line transform of length n under _axis_plan(n) (include/ocpg_hip.h, ocpg_lfm_spectrum_fwd_any), formed in fp64:
    float2 exp(-2 pi i m / n) [n]; the s-point DFT matrix of every stage 1 < s <= 16 in plan order; int32 [n], the slot of element k."""
    from ....util.misc import memo

    def make():
        plan = _axis_plan(n)

        def angles(idx, m):
            a = idx.to(torch.float64) * (-2.0 * torch.pi / m)
            return torch.stack([a.cos(), a.sin()], -1)
        parts = [angles(torch.arange(n), n)]
        for r in plan:
            if 1 < r <= _MAXR:
                k = torch.arange(r)
                parts.append(angles((k[:, None] * k[None, :]).remainder(r).flatten(), r))
        s0, s1, s2 = ([r for r in plan if r != 1] + [1, 1, 1])[:3]
        k = torch.arange(n)
        slot = ((k % s0) * s1 + (k // s0) % s1) * s2 + k // (s0 * s1)
        return torch.cat([torch.cat(parts).float().flatten(), slot.to(torch.int32).view(torch.float32)]).contiguous().to(device)
    return memo("lfm_tw_any", n, device, make)


# ---- a chirp-z (Bluestein) line transform for any length 65..128 (csrc/lfm_dft_czt.hip) -------------------------------------------------
CZT_MIN, CZT_MAX, CZT_M = 65, 128, 256      # the chirp lengths and the length of the cyclic convolution that serves them
# channels per workgroup of a pass along a chirp axis (64 only in a diagnostic build of csrc/lfm_dft_czt.hip with -DOCPG_CZT_CHW=64)
CZT_SLAB = 64 if "-DOCPG_CZT_CHW=64" in os.environ.get("OCPG_HIPCC_FLAGS", "").split() else 32


def _twiddles_czt(n, device):
    """The table of a chirp axis of length n (include/ocpg_hip.h, ocpg_lfm_spectrum_fwd_czt), formed in fp64: float2 [896] = the chirp
    c_m = exp(-i pi m^2 / n) [128, zero from n on]; the forward B = FFT_256(wrapped conj(c)) / 256 and the inverse B = FFT_256(wrapped c) /
    256, both [256] with entry 16 k1 + k2 holding B[k1 + 16 k2]; exp(-2 pi i m / 256) [256].  The chirp's angle is reduced as m^2 mod 2n
    in integers first."""
    from ....util.misc import memo

    def make():
        assert CZT_MIN <= n <= CZT_MAX, n
        m = torch.arange(n, dtype=torch.int64)
        a = ((m * m) % (2 * n)).to(torch.float64) * (-torch.pi / n)
        c = torch.complex(a.cos(), a.sin())
        wrapped = torch.zeros(CZT_M, dtype=torch.complex128)
        wrapped[:n] = c.conj()
        wrapped[CZT_M - n + 1:] = c.conj()[1:].flip(0)
        k = torch.arange(CZT_M)
        order = (k // 16) + 16 * (k % 16)                 # entry 16 k1 + k2 <- element k1 + 16 k2
        bf = torch.fft.fft(wrapped)[order] / CZT_M
        bi = torch.fft.fft(wrapped.conj())[order] / CZT_M
        w = torch.arange(CZT_M, dtype=torch.float64) * (-2.0 * torch.pi / CZT_M)
        cpad = torch.zeros(CZT_MAX, dtype=torch.complex128)
        cpad[:n] = c
        table = torch.cat([cpad, bf, bi, torch.complex(w.cos(), w.sin())])
        return torch.view_as_real(table).float().contiguous().to(device)
    return memo("lfm_tw_czt", n, device, make)


def _route(h, w):
    """0: csrc/lfm_dft.hip serves the map; 1: csrc/lfm_dft_any.hip does; raises when neither."""
    if dft_supported(h, w):
        return 0
    if not dft_any_supported(h, w):
        raise RuntimeError(f"LFM transforms: a {h} x {w} map is served by neither csrc/lfm_dft.hip nor csrc/lfm_dft_any.hip")
    return 1


def _slab(length):
    return 32 if length > 128 else 64          # channels per workgroup of a pass along an axis of this length (lfm_dft_any.hip)


def _nhwc32(x):
    """[N, C, h, w] -> its channels-last memory as an fp32 [N, h, w, C] contiguous tensor (a view when it already is)."""
    v = x.permute(0, 2, 3, 1)
    if v.dtype != torch.float32:
        v = v.float()
    return v if v.is_contiguous() else v.contiguous()


def _pair_cl(y):
    v = y.permute(0, 2, 3, 1)
    if v.dtype not in _DT:
        v = v.float()
    return v if v.is_contiguous() else v.contiguous()


def _czt_args(h, w, czt, dev):
    """What the _czt entries get after the arguments of the _any entries' tables: (tw_h, tw_w, plans..., cz_h, cz_w).  A chirp axis has the
    plan (1, 1, L) and its chirp table (also handed over as its tw, which is not read); the other axis its _any table and _axis_plan."""
    tw, plans, cz = [], [], []
    for length, on in ((h, czt[0]), (w, czt[1])):
        if on:
            if not CZT_MIN <= length <= CZT_MAX:
                raise RuntimeError(f"LFM transforms: a chirp axis of length {length} is outside {CZT_MIN}..{CZT_MAX}")
            t = _twiddles_czt(length, dev)
            tw.append(t.data_ptr()), plans.extend((1, 1, length)), cz.append(t.data_ptr())
        else:
            if dft_plan(length) is None:
                raise RuntimeError(f"LFM transforms: an axis of length {length} beside a chirp axis is not served by csrc/lfm_dft_any.hip")
            tw.append(_twiddles_any(length, dev).data_ptr()), plans.extend(_axis_plan(length)), cz.append(None)
    return tw, plans, cz


def _spectrum(x_nhwc, coef, high, norm, dtype, czt=(False, False)):
    n, h, w, c = x_nhwc.shape
    dev = x_nhwc.device
    czt = (bool(czt[0]), bool(czt[1]))
    any_ = 2 if any(czt) else _route(h, w)
    tmp = torch.empty((n, h, w // 2 + 1, c, 2), dtype=torch.float32, device=dev)
    pair = torch.empty((n, h, w, 2 * c), dtype=dtype, device=dev)
    args = (x_nhwc.data_ptr(), coef.data_ptr() if coef is not None else None, high.data_ptr() if high is not None else None, n, h, w, c)
    if any_ == 2:
        tw, plans, cz = _czt_args(h, w, czt, dev)
        check(lib().ocpg_lfm_spectrum_fwd_czt(*args, *tw, float(norm), tmp.data_ptr(), pair.data_ptr(), _DT[dtype], *plans, *cz,
                                              torch.cuda.current_stream().cuda_stream), "ocpg_lfm_spectrum_fwd_czt")
    elif any_:
        check(lib().ocpg_lfm_spectrum_fwd_any(*args, _twiddles_any(h, dev).data_ptr(), _twiddles_any(w, dev).data_ptr(), float(norm), tmp.data_ptr(),
                                              pair.data_ptr(), _DT[dtype], *_axis_plan(h), *_axis_plan(w), torch.cuda.current_stream().cuda_stream),
              "ocpg_lfm_spectrum_fwd_any")
    else:
        check(lib().ocpg_lfm_spectrum_fwd(*args, _twiddles(h, dev).data_ptr(), _twiddles(w, dev).data_ptr(), float(norm), tmp.data_ptr(),
                                          pair.data_ptr(), _DT[dtype], torch.cuda.current_stream().cuda_stream), "ocpg_lfm_spectrum_fwd")
    return pair


def _inverse(pair, coef, high, z_saved, want_coef, norm, residual, czt=(False, False)):
    n, h, w, c2 = pair.shape
    c = c2 // 2
    dev = pair.device
    czt = (bool(czt[0]), bool(czt[1]))
    any_ = 2 if any(czt) else _route(h, w)
    slab = CZT_SLAB if czt[0] else _slab(h) if any_ else 64
    tmp = torch.empty((n, h, w // 2 + 1, c, 2), dtype=torch.float32, device=dev)
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
    part = torch.empty((n, (w // 2 + 1) * ((c + slab - 1) // slab)), dtype=torch.float32, device=dev) if want_coef else None
    args = (pair.data_ptr(), _DT[pair.dtype], coef.data_ptr() if coef is not None else None, high.data_ptr() if high is not None else None,
            z_saved.data_ptr() if want_coef else None, part.data_ptr() if want_coef else None, n, h, w, c)
    tail = (float(norm), tmp.data_ptr(), residual.data_ptr() if residual is not None else None, out.data_ptr())
    if any_ == 2:
        tw, plans, cz = _czt_args(h, w, czt, dev)
        check(lib().ocpg_lfm_spectrum_inv_czt(*args, *tw, *tail, *plans, *cz, torch.cuda.current_stream().cuda_stream), "ocpg_lfm_spectrum_inv_czt")
    elif any_:
        check(lib().ocpg_lfm_spectrum_inv_any(*args, _twiddles_any(h, dev).data_ptr(), _twiddles_any(w, dev).data_ptr(), *tail, *_axis_plan(h),
                                              *_axis_plan(w), torch.cuda.current_stream().cuda_stream), "ocpg_lfm_spectrum_inv_any")
    else:
        check(lib().ocpg_lfm_spectrum_inv(*args, _twiddles(h, dev).data_ptr(), _twiddles(w, dev).data_ptr(), *tail,
                                          torch.cuda.current_stream().cuda_stream), "ocpg_lfm_spectrum_inv")
    return out, part


class LFMSpectrum(Function):
    """z = cat([Re, Im], 1)(fft2(x) * (1 - coef * high)) of a real map (models/modules.py:44-50) as a [N, 2C, h, w] tensor in
    channels-last memory and the 1x1 convs' compute dtype: two passes of csrc/lfm_dft.hip (csrc/lfm_dft_any.hip for a map that one refuses).  Backward: the real part of the unnormalised
    inverse transform of gate * gz, and the gate coefficient's gradient from the saved z."""

    @staticmethod
    def forward(ctx, x, coef, high, dtype, czt=(False, False)):
        xs = _nhwc32(x)
        coef, high = coef.float().contiguous(), high.float().contiguous()
        pair = _spectrum(xs, coef, high, 1.0, dtype, czt)
        ctx.save_for_backward(pair, coef, high)
        ctx.czt = czt
        return pair.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        pair, coef, high = ctx.saved_tensors
        g = _pair_cl(gz)
        if g.dtype != pair.dtype:
            g = g.to(pair.dtype)
        want_coef = ctx.needs_input_grad[1]
        gx, part = _inverse(g, coef, high, pair, want_coef, 1.0, None, ctx.czt)
        return gx.permute(0, 3, 1, 2), (part.sum(1) if want_coef else None), None, None, None


class LFMInverse(Function):
    """x + ifft2(complex(y[:, :C], y[:, C:]), s=(h, w)).real (models/modules.py:52-56) for y in channels-last memory, as two passes of
    csrc/lfm_dft.hip; fp32 result in channels-last memory.  Backward: fft2(g) / (h w) as a [Re || Im] pair in y's dtype; g for x."""

    @staticmethod
    def forward(ctx, y, x, czt=(False, False)):
        ys, xs = _pair_cl(y), _nhwc32(x)
        n, h, w, _ = ys.shape
        out, _ = _inverse(ys, None, None, None, False, 1.0 / (h * w), xs, czt)
        ctx.dtype = (y.dtype, ys.dtype)
        ctx.czt = czt
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ydt, sdt = ctx.dtype
        gy = None
        if ctx.needs_input_grad[0]:
            gs = _nhwc32(g)
            n, h, w, _ = gs.shape
            gy = _spectrum(gs, None, None, 1.0 / (h * w), sdt, ctx.czt).permute(0, 3, 1, 2)
            if gy.dtype != ydt:
                gy = gy.to(ydt)
        return gy, (g if ctx.needs_input_grad[1] else None), None


def lfm_spectrum(x, coef, high, dtype, czt=(False, False)):
    """czt = (h, w): the axes that run the chirp-z line transform of csrc/lfm_dft_czt.hip (a length 65..128 each); the backward pass follows."""
    return LFMSpectrum.apply(x, coef, high, dtype, (bool(czt[0]), bool(czt[1])))


def lfm_inverse(y, x, czt=(False, False)):
    return LFMInverse.apply(y, x, (bool(czt[0]), bool(czt[1])))
