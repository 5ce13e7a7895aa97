"""LFMResizeAdaptive -- the spectral (low-frequency modulation) block used before and after text fusion.

Follows the reference's models/modules.py:9-61: a 3x3 *valid* "laplace" conv -> global average -> FC -> sigmoid
gives one coefficient per sample; the 2-D spectrum of the map is attenuated by (1 - coef * gaussian) where the
Gaussian (sigma 7) is centred at (h//2, w//2) of the UNSHIFTED spectrum and, once created at the first level, is
bilinearly resized for every later call; two 1x1 convs act on [real || imag]; inverse FFT; residual.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ..util.misc import memo
from . import amp_cache, fallbacks
import os

from .ops.functions.spectral_func import (CZT_MAX, CZT_MIN, conv3x3_valid_spatial_mean, dft_any_supported, dft_plan, dft_supported, ifft2_real, lfm_inverse,
                                          lfm_spectrum, pair_to_complex, spectral_gate, spectral_gate_cl)

FUSED_GATE = True       # A/B switch: fused spectral gate kernel
GATE_NHWC = True        # A/B switch: gate output / inverse-FFT input in channels-last memory (1x1 convs as GEMMs, no casts / layout copies)
DFT_CL = os.environ.get("OCPG_LFM_DFT", "1") != "0"       # A/B switch: both transforms by csrc/lfm_dft.hip on the channels-last map (else rocFFT between transposes)
# OCPG_LFM_DFT_ANY (default 1): a map csrc/lfm_dft.hip refuses (a length with a prime factor > 16, 125, or above 128) runs both transforms on
# csrc/lfm_dft_any.hip instead of rocFFT; 0 restores the library route for those maps exactly.  DFT_ANY_MAX_PRIME: the largest prime factor
# whose direct O(p^2) stage is not slower than the library route (measured, DESIGN 4.8x: profiles/lfm_dft_any_ab.jsonl); a map with a larger one
# (or a length above 256) goes to the library and is counted in models/fallbacks.py.  The kernels themselves serve every prime up to 251.
DFT_ANY = os.environ.get("OCPG_LFM_DFT_ANY", "1") != "0"
DFT_ANY_MAX_PRIME = 79


def dft_any_default(length):
    """Does a line of this length take csrc/lfm_dft_any.hip by default?  Yes when its plan has stages <= 16 only (every such length up to 256
    measured faster), or one prime stage <= DFT_ANY_MAX_PRIME in a length <= 128 (above 128 a workgroup runs 32 channels with half of each
    wave idle in the stages, and the direct stage then loses to the library at every prime measured)."""
    plan = dft_plan(length)
    if plan is None:
        return False
    return max(plan) <= 16 or (max(plan) <= DFT_ANY_MAX_PRIME and length <= 128)


# OCPG_LFM_DFT_CZT (default 1): a PRIME axis length p with DFT_CZT_MIN_PRIME <= p <= 127 runs the chirp-z line transform of csrc/lfm_dft_czt.hip
# (the other axis: one the kernels above take by default, or a chirp axis itself); 0 restores the routing without it exactly, counted fallbacks
# included; "force" sends every prime 67..127 to the chirp axis.  DFT_CZT_MIN_PRIME: the smallest prime from which the chirp route beat both the
# library route and the direct stage on both axes, at that prime and every larger one (measured, DESIGN 4.8y: profiles/lfm_dft_czt_ab.jsonl);
# None: no prime did, and the kernels stay behind "force".
_CZT_ENV = os.environ.get("OCPG_LFM_DFT_CZT", "1")
DFT_CZT = _CZT_ENV != "0"
DFT_CZT_FORCE = _CZT_ENV == "force"
DFT_CZT_MIN_PRIME = 67
_CZT_FORCE_MIN = 67


def _is_prime(v):
    return v >= 2 and all(v % d for d in range(2, int(v ** 0.5) + 1))


def dft_czt_axis(length):
    """Is a line of this length a chirp axis under the switches as they stand?"""
    if not DFT_CZT or not (CZT_MIN <= length <= min(CZT_MAX, 127)) or not _is_prime(length):
        return False
    lo = _CZT_FORCE_MIN if DFT_CZT_FORCE else DFT_CZT_MIN_PRIME
    return lo is not None and length >= lo


def _czt_range():
    lo = _CZT_FORCE_MIN if DFT_CZT_FORCE else DFT_CZT_MIN_PRIME
    return f"{lo}..127" if DFT_CZT and lo is not None else "(none: the chirp route is off)"


def dft_route(h, w):
    """Who runs both transforms of an h x w map, and the chirp axes (h, w): "old" csrc/lfm_dft.hip, "any" csrc/lfm_dft_any.hip, "czt"
    csrc/lfm_dft_czt.hip, "library" rocFFT between transposing copies (a counted fallback when DFT_ANY is on).  Pure: reads the switches only."""
    none = (False, False)
    if not DFT_CL:
        return "library", none
    if dft_supported(h, w):
        return "old", none
    if not DFT_ANY:
        return "library", none
    axes = (dft_czt_axis(h), dft_czt_axis(w))
    if any(axes) and all(on or dft_any_default(length) for on, length in zip(axes, (h, w))):
        return "czt", axes
    if dft_any_supported(h, w) and dft_any_default(h) and dft_any_default(w):
        return "any", none
    return "library", none


LAPLACE_MEAN = True   # A/B switch: mean(laplace(x)) as nine window means + one small matrix product (no convolution)


class LFMResizeAdaptive(nn.Module):
    def __init__(self, num_channels, sigma):
        super().__init__()
        self.conv1 = amp_cache.Conv2d(2 * num_channels, 2 * num_channels, kernel_size=1)
        self.conv2 = amp_cache.Conv2d(2 * num_channels, 2 * num_channels, kernel_size=1)
        amp_cache.mark_single_use(self.conv1, self.conv2)       # applied once per forward: their gradient sums ride in the fused cast
        self.sigma = sigma
        self.laplace = amp_cache.Conv2d(num_channels, num_channels, kernel_size=3, padding=0)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(amp_cache.Linear(num_channels, num_channels, bias=False), nn.ReLU(inplace=True),
                                amp_cache.Linear(num_channels, 1, bias=False), nn.Sigmoid())

    @staticmethod
    def make_gaussian(cy, cx, height, width, sigma=7, device="cpu"):
        ys = torch.arange(height, dtype=torch.float32, device=device).view(-1, 1)
        xs = torch.arange(width, dtype=torch.float32, device=device).view(1, -1)
        return torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * sigma ** 2))[None, None]

    def forward(self, x, gauss_map=None):
        # Precision follows the reference exactly: the input and the FFTs are fp32 (`x.float()`, modules.py:35), while the
        # three convs / two FCs are ordinary autocast ops (fp16 in the reference's --amp runs, bf16 here) whose outputs
        # are cast back with `.float()` (modules.py:56).  Without autocast everything is fp32.
        b, c, h, w = x.shape
        x = x.float()
        if x.is_cuda and LAPLACE_MEAN and self.laplace.kernel_size == (3, 3) and self.laplace.padding == (0, 0):
            # the spatial mean of a convolution is linear in its input (csrc/lfm.hip): same products, no 3x3 convolution
            amp = torch.is_autocast_enabled("cuda")
            wl, bl = amp_cache.lookup(self.laplace.weight), amp_cache.lookup(self.laplace.bias)
            if amp:
                dt = torch.get_autocast_dtype("cuda")
                wl, bl = wl.to(dt), bl.to(dt)
            lap_mean = conv3x3_valid_spatial_mean(x, wl, bl, amp and wl.dtype == torch.bfloat16)
            if amp:
                lap_mean = lap_mean.to(wl.dtype)          # the dtype the autocast convolution + mean would have produced
        else:
            lap_mean = self.laplace(x).mean(dim=(2, 3))
        coef = self.fc(lap_mean).view(b, 1, 1, 1)
        # the Gaussian of level 0 and its chain of bilinear resizes depend only on the map sizes: memoised (util.misc.memo)
        if gauss_map is None:
            key = ("gauss", h // 2, w // 2, h, w, float(self.sigma))
            high = memo("lfm_gauss", key, x.device, lambda: self.make_gaussian(h // 2, w // 2, h, w, self.sigma, x.device))
        else:
            parent = getattr(gauss_map, "_ocpg_key", None)
            key = None if parent is None else ("resized", parent, h, w)
            high = memo("lfm_gauss", key, x.device, lambda: F.interpolate(gauss_map, size=(h, w), mode="bilinear", align_corners=False))
        if key is not None:
            high._ocpg_key = key
        if x.is_cuda and FUSED_GATE and GATE_NHWC and c % 4 == 0:
            dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
            route, czt = dft_route(h, w)
            if route == "library" and DFT_CL and DFT_ANY:
                # counted (and an error under OCPG_STRICT_HIP=1); silent only with the switch off
                fallbacks.note("LFM", f"no own Fourier transform for a {h} x {w} map by default (a length above 256, a prime factor above "
                                      f"{DFT_ANY_MAX_PRIME} that is not a chirp-axis prime {_czt_range()}, or one above 16 in a length above 128)", x)
            if route != "library":
                z = lfm_spectrum(x, coef.float().reshape(b), high.reshape(h, w), dt, czt)      # fft2 + gate + [Re || Im], channels-last
                y = self.conv2(F.relu(self.conv1(z)))
                return lfm_inverse(y, x, czt), high                                          # x + ifft2(.).real
            z = spectral_gate_cl(torch.fft.fft2(x), coef.float().reshape(b), high.reshape(h, w), dt)
            y = self.conv2(F.relu(self.conv1(z)))                   # channels-last in, channels-last out: two GEMMs
            y = ifft2_real(pair_to_complex(y), h, w)              # = torch.fft.ifft2(..., s=(h, w)).real, real-to-complex backward
            return x + y, high
        if x.is_cuda and FUSED_GATE:
            # gate, real/imag split and concatenation in one pass (csrc/spectral.hip)
            z = spectral_gate(torch.fft.fft2(x), coef.float().reshape(b), high.reshape(h, w))
        else:
            spec = torch.fft.fft2(x) * (1 - coef.float() * high)
            z = torch.cat([spec.real, spec.imag], dim=1)
        y = self.conv2(F.relu(self.conv1(z))).float()
        yr, yi = torch.chunk(y, 2, dim=1)
        y = torch.fft.ifft2(torch.complex(yr, yi), s=(h, w)).real.float()
        return x + y, high
