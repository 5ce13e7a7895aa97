"""Input front end of a clip: binding of ocpg_clip_front_u8 (csrc/clip_front.hip).

The reference resizes every frame with Pillow (torchvision F.resize on a PIL image = Image.resize((w, h), BILINEAR)): a horizontal and
a vertical pass of integer arithmetic on coefficient tables, each pass rounded to uint8.  `resample_tables` restates Pillow's
precompute_coeffs / normalize_coeffs_8bpc in fp64 on the host; the two passes on those tables are pure int32, so `clip_front` returns
Pillow's bytes exactly -- optionally of a crop window, flipped, normalised (ToTensor + Normalize as a 3 x 256 table filled by
normalize_clip itself) and written into a strided destination such as a clip's slot of the padded batch.  GPU tensors run the one HIP
kernel; CPU tensors run a torch integer composition of the same two passes, so the host logic stays testable without a GPU.
"""
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from ...._lib import check, lib, stream_ptr

PRECISION_BITS = 22
LDS_BYTES = 32768           # dynamic LDS a launch may ask for (csrc/clip_front.hip: MAX_LDS)
TILE_W = 64                 # bytes per LDS row = output columns per workgroup


@functools.lru_cache(maxsize=1024)
def resample_tables(in_size: int, out_size: int):
    """-> (bounds int32 [out, 2] = (first tap, taps), coefs int32 [out, ksize], ksize) of Pillow's bilinear filter for one axis
    (Resample.c: precompute_coeffs with the triangle filter, normalize_coeffs_8bpc), in numpy float64 = C doubles, every operation in
    Pillow's order; the loop runs over the taps, so each output index adds its weights one after another as Pillow does (a tap beyond
    the index's count adds 0.0, which changes nothing).  The arrays are read-only (cached)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                      # the cast truncates, as C's (int)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        v = np.abs(((x + xmin) - center + 0.5) * ss)
        v = np.where((v < 1.0) & (x < xmax), 1.0 - v, 0.0)
        w[:, x] = v
        ww += v
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    coefs = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)         # the triangle filter has no negative weights
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    coefs.setflags(write=False)
    return bounds, coefs, ksize


@functools.lru_cache(maxsize=1024)
def tile_rows(in_size: int, out_size: int):
    """-> (TR, rows): the largest TR of 16, 8, 4, 2, 1 output rows per workgroup whose worst tile's source rows (first tap of its first
    row .. last tap of its last row) fit LDS_BYTES as uint8 rows of TILE_W, and that worst row count."""
    bounds, _, _ = resample_tables(in_size, out_size)
    first, last = bounds[:, 0].astype(np.int64), bounds[:, 0].astype(np.int64) + bounds[:, 1]
    for tr in (16, 8, 4, 2, 1):
        a = np.arange(0, out_size, tr)
        b = np.minimum(a + tr, out_size) - 1
        rows = int((last[b] - first[a]).max())
        if rows * TILE_W <= LDS_BYTES:
            return tr, max(rows, 1)
    raise ValueError(f"clip_front: a {in_size} -> {out_size} resize needs {rows} source rows for one output row; "
                     f"at most {LDS_BYTES // TILE_W} are served")


_DEVICE_TABLES = OrderedDict()
_DEVICE_TABLES_CAP = 1024
_LUTS = {}


def device_tables(in_size: int, out_size: int, device):
    """resample_tables as device tensors, one upload per (sizes, device), kept for the most recent _DEVICE_TABLES_CAP pairs: resident
    before a graph capture that uses them."""
    key = (int(in_size), int(out_size), str(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        bounds, coefs, ksize = resample_tables(in_size, out_size)
        both = torch.from_numpy(np.concatenate([bounds.reshape(-1), coefs.reshape(-1)])).to(device)
        t = (both[:bounds.size], both[bounds.size:], ksize)
        _DEVICE_TABLES[key] = t
        if len(_DEVICE_TABLES) > _DEVICE_TABLES_CAP:
            _DEVICE_TABLES.popitem(last=False)
    else:
        _DEVICE_TABLES.move_to_end(key)
    return t


def normalize_lut(device):
    """fp32 [3 * 256]: normalize_clip of every byte value per channel -- the kernel's mode 1 is then bit-equal to the torch composition."""
    key = str(device)
    t = _LUTS.get(key)
    if t is None:
        from ....datasets.clip_transforms import normalize_clip
        ramp = torch.arange(256, dtype=torch.uint8).view(1, 1, 1, 256).expand(1, 3, 1, 256)
        t = normalize_clip(ramp, None)[0].reshape(3 * 256).contiguous().to(device)
        _LUTS[key] = t
    return t


def _pass_cpu(x, bounds, coefs, dim):
    """One Pillow pass over `dim` of an int32 tensor of bytes: gathers of the taps, int32 accumulation, round, clip."""
    b = torch.from_numpy(bounds.copy()).to(torch.int64)            # the cached arrays are read-only: copy before wrapping
    k = torch.from_numpy(coefs.copy())
    size = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = b.shape[0]
    acc = None
    for t in range(k.shape[1]):
        if not bool((k[:, t] != 0).any()):
            continue
        idx = (b[:, 0] + t).clamp(max=size - 1)            # taps beyond a row's count carry weight 0
        term = x.index_select(dim, idx) * k[:, t].view(shape)
        acc = term if acc is None else acc + term
    return ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp(0, 255)


def _check_geometry(clip, out_hw, window):
    if clip.dim() != 4 or clip.shape[1] != 3:
        raise ValueError(f"clip_front: expected a [T, 3, H, W] clip, got {tuple(clip.shape)}")
    if clip.dtype != torch.uint8:
        raise ValueError(f"clip_front: expected a uint8 clip (Pillow's 8-bit resample), got {clip.dtype}")
    h, w = clip.shape[-2:]
    top, left, wh, ww = (0, 0, h, w) if window is None else (int(v) for v in window)
    if not (0 <= top and 0 <= left and 1 <= wh and 1 <= ww and top + wh <= h and left + ww <= w):
        raise ValueError(f"clip_front: window {(top, left, wh, ww)} outside the {h} x {w} frame")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh < 1 or ow < 1:
        raise ValueError(f"clip_front: output size {(oh, ow)} must be positive")
    return (top, left, wh, ww), (oh, ow)


def _plane_strides(t):
    """[T, 3, h, w] tensor -> (plane stride, row stride) in elements, or None when its planes are not evenly spaced rows of
    contiguous elements."""
    st, sc, sh, sw = t.stride()
    if (t.shape[-1] > 1 and sw != 1) or (t.shape[0] > 1 and st != 3 * sc) or sc <= 0 or sh <= 0:
        return None
    return sc, sh


@torch.no_grad()
def clip_front(clip_u8, out_hw, window=None, flip=False, normalize=False, out=None):
    """clip_u8 [T, 3, H, W] uint8 -> [T, 3, oh, ow]: Image.resize((ow, oh), BILINEAR) of every frame's `window` = (top, left, h, w)
    (default: the whole frame; the window is the image that is resized, as after F.crop), flipped left-right with flip=True; uint8,
    or with normalize=True fp32 = normalize_clip of those bytes.  out: a [T, 3, oh, ow] tensor or view (last axis contiguous, planes
    evenly spaced, e.g. batch[b, :T, :, :oh, :ow]) that is filled instead; nothing outside it is written."""
    (top, left, wh, ww), (oh, ow) = _check_geometry(clip_u8, out_hw, window)
    n = clip_u8.shape[0]
    dtype = torch.float32 if normalize else torch.uint8
    if out is None:
        out = torch.empty((n, 3, oh, ow), dtype=dtype, device=clip_u8.device)
    elif tuple(out.shape) != (n, 3, oh, ow) or out.dtype != dtype or out.device != clip_u8.device:
        raise ValueError(f"clip_front: out must be {(n, 3, oh, ow)} {dtype} on {clip_u8.device}, "
                         f"got {tuple(out.shape)} {out.dtype} on {out.device}")
    if n == 0:
        return out
    if not clip_u8.is_cuda:
        by, ky, _ = resample_tables(wh, oh)
        bx, kx, _ = resample_tables(ww, ow)
        x = clip_u8[:, :, top:top + wh, left:left + ww].to(torch.int32)
        x = _pass_cpu(_pass_cpu(x, bx, kx, 3), by, ky, 2)
        if flip:
            x = x.flip(-1)
        if normalize:
            x = normalize_lut(x.device).view(1, 3, 256).expand(n, 3, 256).gather(2, x.reshape(n, 3, oh * ow).to(torch.int64)).view(n, 3, oh, ow)
        out.copy_(x.to(dtype))
        return out
    if _plane_strides(clip_u8) is None:
        clip_u8 = clip_u8.contiguous()
    src_plane, src_row = _plane_strides(clip_u8)
    strides = _plane_strides(out)
    if strides is None:
        raise ValueError(f"clip_front: out needs a contiguous last axis and evenly spaced planes, got strides {out.stride()}")
    tr, cap = tile_rows(wh, oh)
    by, ky, ksy = device_tables(wh, oh, clip_u8.device)
    bx, kx, ksx = device_tables(ww, ow, clip_u8.device)
    lut = normalize_lut(clip_u8.device) if normalize else None
    with torch.cuda.device(clip_u8.device):
        check(lib().ocpg_clip_front_u8(clip_u8.data_ptr(), n * 3, src_plane, src_row, clip_u8.shape[2], clip_u8.shape[3], top, left, wh, ww,
                                       by.data_ptr(), ky.data_ptr(), ksy, bx.data_ptr(), kx.data_ptr(), ksx, oh, ow, int(bool(flip)),
                                       1 if normalize else 0, tr, cap, out.data_ptr(), strides[0], strides[1],
                                       None if lut is None else lut.data_ptr(), stream_ptr()), "ocpg_clip_front_u8")
    return out
