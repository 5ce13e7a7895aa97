"""Mask-head front end: autograd binding of csrc/mask_front.hip.

`memfuse(memory, shapes, n_lvl, ...)`: the memory fusion x_0 + R_1 x_1 + R_2 x_2 (bicubic, align_corners=False) read from the token-major
encoder output [N, S, C] as it lies and written as NCHW (the dynamic mask head's operand) and / or channels-last (ls_feat_viz's
operand): one launch forward, one backward, in place of the three permute copies, the four matmuls (eight with the backward), the
channels-last copy, the slice backwards and the strided add of the two consumers' gradients.

`lsfeat(lsf, txt, frames, b, t, size)`: the level-set feature stack [b, t, 12, 4h, 4w] (bilinear frames, bilinear x4 of ls_feat_viz's
output read in the dtype it arrives in, sim) written directly, one launch forward and one backward (+ one small sum for txt), in place
of ~25 ATen ops forward and ~50 backward; a zero gradient on the sim channel costs nothing and gives txt exactly 0.

The resampling weights are the 1-D matrices `resample.bicubic_matrix` builds, the operands of the matmuls this op replaces; next to
them the kernels get, per output index and per source index, the range of the entries that are not zero.  `LevelMaps` is what
DeformableTransformer.forward returns in place of the list of NCHW copies: the memory, its level shapes, and the copies on demand.
"""
import os
from collections import OrderedDict

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import DTYPE_CODE as _DT, check, lib, stream_ptr
from ...resample import bicubic_matrix, bilinear_matrix

# A/B switch, read once: 1 = memory fusion and level-set feature stack by csrc/mask_front.hip on the GPU training path; 0 = the torch lines
ENABLED = os.environ.get("OCPG_MASK_FRONT", "1") != "0"
NOT_SERVED = -2000
_TABLES = OrderedDict()         # geometry -> device tables, least recently used first, at most _TABLES_MAX entries
_TABLES_MAX = 64


def _cached(key, build):
    if key in _TABLES:
        _TABLES.move_to_end(key)
    else:
        _TABLES[key] = build()
        while len(_TABLES) > _TABLES_MAX:
            _TABLES.popitem(last=False)
    return _TABLES[key]


def _dev_key(device):
    device = torch.device(device)
    return (device.type, torch.cuda.current_device() if device.type == "cuda" and device.index is None else device.index)


class LevelMaps:
    """The first `n` levels of a token-major memory [N, S, C] as a sequence of NCHW maps, copied out only when someone indexes it."""

    def __init__(self, memory, shapes, n):
        self.memory, self.shapes, self.n = memory, tuple(tuple(int(v) for v in s) for s in shapes), n
        self._maps = None

    def maps(self):
        if self._maps is None:
            nb, _, c = self.memory.shape
            self._maps, start = [], 0
            for (h, w) in self.shapes[:self.n]:
                self._maps.append(self.memory[:, start:start + h * w].reshape(nb, h, w, c).permute(0, 3, 1, 2).contiguous())
                start += h * w
        return self._maps

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.maps()[i]

    def __iter__(self):
        return iter(self.maps())


def _ranges(nz):
    """nz [rows, cols] bool -> int32 [rows, 2]: first True column and the count up to the last True one (0, 0 for an empty row)."""
    cols = nz.shape[1]
    idx = torch.arange(cols)
    first = torch.where(nz, idx, torch.full_like(idx, cols)).min(1).values
    last = torch.where(nz, idx, torch.full_like(idx, -1)).max(1).values
    cnt = (last - first + 1).clamp(min=0)
    return torch.stack([first.clamp(max=cols - 1), cnt], 1).to(torch.int32)


def tables(shapes, n_lvl, device):
    """(wts, rng, geom): the device tables of csrc/mask_front.hip for these level shapes and their host-side directory, cached per
    geometry and device: nothing is copied to the device after the first step (capturable)."""
    def build():
        (h0, w0) = shapes[0]
        wts, rng, geom, start = [], [], [], 0
        wn = rn = 0
        for l, (h, w) in enumerate(shapes):
            row = [h, w, start, 0, 0, 0, 0, 0, 0]
            start += h * w
            if 1 <= l < n_lvl:
                my, mx = bicubic_matrix(h, h0, "cpu"), bicubic_matrix(w, w0, "cpu")          # [h0, h], [w0, w]
                for k, m in ((3, my), (4, mx)):
                    row[k] = wn
                    wts.append(m.reshape(-1))
                    wn += m.numel()
                for k, r in ((5, _ranges(my != 0)), (6, _ranges(mx != 0)), (7, _ranges(my.t() != 0)), (8, _ranges(mx.t() != 0))):
                    row[k] = rn
                    rng.append(r.reshape(-1))
                    rn += r.numel()
            geom.append(row)
        wts_t = torch.cat(wts) if wts else torch.zeros(1)
        rng_t = torch.cat(rng) if rng else torch.zeros(2, dtype=torch.int32)
        return wts_t.to(device), rng_t.to(device), torch.tensor(geom, dtype=torch.int64)
    return _cached(("memfuse", shapes, n_lvl, _dev_key(device)), build)


def _two_taps(n_in, n_out):
    """bilinear_matrix(align_corners=True) as per-output (first source index [n_out] int32, the two matrix entries [n_out, 2])."""
    m = bilinear_matrix(n_in, n_out, True, "cpu")
    r = _ranges(m != 0)
    lo = r[:, 0].long()
    nxt = (lo + 1).clamp(max=n_in - 1)
    w1 = torch.where(lo + 1 < n_in, m.gather(1, nxt[:, None])[:, 0], torch.zeros(n_out))
    return r[:, 0].contiguous(), torch.stack([m.gather(1, lo[:, None])[:, 0], w1], 1), m


def ls_tables(h, w, H, W, Ho, Wo, device):
    """(tab_i, tab_w, off): the device tables of the level-set feature kernels and their host directory, cached per geometry."""
    def build():
        ly_i, ly_w, my = _two_taps(h, Ho)
        lx_i, lx_w, mx = _two_taps(w, Wo)
        fy_i, fy_w, _ = _two_taps(H, Ho)
        fx_i, fx_w, _ = _two_taps(W, Wo)
        ints = [ly_i, lx_i, fy_i, fx_i, _ranges(my.t() != 0).reshape(-1), _ranges(mx.t() != 0).reshape(-1)]
        flts = [ly_w.reshape(-1), lx_w.reshape(-1), fy_w.reshape(-1), fx_w.reshape(-1)]
        off, n = [], 0
        for t in ints:
            off.append(n)
            n += t.numel()
        ni, n = n, 0
        for t in flts:
            off.append(n)
            n += t.numel()
        return torch.cat(ints).to(torch.int32).to(device), torch.cat(flts).float().to(device), torch.tensor(off + [ni, n], dtype=torch.int64)
    return _cached(("lsfeat", h, w, H, W, Ho, Wo, _dev_key(device)), build)


class _NotServed(Exception):
    pass


class MemFuse(Function):
    @staticmethod
    def forward(ctx, memory, shapes, n_lvl, want_nchw, want_cl):
        ctx.set_materialize_grads(False)
        nb, s, c = memory.shape
        (h0, w0) = shapes[0]
        wts, rng, geom = tables(shapes, n_lvl, memory.device)
        nchw = torch.empty((nb, c, h0, w0), dtype=torch.float32, device=memory.device) if want_nchw else None
        cl = torch.empty((nb, h0, w0, c), dtype=torch.float32, device=memory.device) if want_cl else None
        with torch.cuda.device(memory.device):
            rc = lib().ocpg_memfuse_fwd_f32(memory.data_ptr(), wts.data_ptr(), rng.data_ptr(), geom.data_ptr(), wts.numel(), rng.numel(),
                                            len(shapes), n_lvl, nb, s, c, None if nchw is None else nchw.data_ptr(),
                                            None if cl is None else cl.data_ptr(), stream_ptr())
        if rc == NOT_SERVED:
            raise _NotServed()
        check(rc, "ocpg_memfuse_fwd_f32")
        ctx.meta = (shapes, n_lvl, tuple(memory.shape))
        return nchw, cl

    @staticmethod
    @once_differentiable
    def backward(ctx, g_nchw, g_cl):
        shapes, n_lvl, (nb, s, c) = ctx.meta
        if g_nchw is None and g_cl is None:
            return None, None, None, None, None
        dev = (g_nchw if g_nchw is not None else g_cl).device
        g_nchw = None if g_nchw is None else g_nchw.float().contiguous()
        g_cl = None if g_cl is None else g_cl.float().contiguous()
        wts, rng, geom = tables(shapes, n_lvl, dev)
        g_mem = torch.empty((nb, s, c), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib().ocpg_memfuse_bwd_f32(None if g_nchw is None else g_nchw.data_ptr(), None if g_cl is None else g_cl.data_ptr(),
                                             wts.data_ptr(), rng.data_ptr(), geom.data_ptr(), wts.numel(), rng.numel(), len(shapes), n_lvl,
                                             nb, s, c, g_mem.data_ptr(), stream_ptr()), "ocpg_memfuse_bwd_f32")
        return g_mem, None, None, None, None


def memfuse(memory, shapes, n_lvl, want_nchw=True, want_cl=True):
    """memory [N, S, C] fp32 GPU, contiguous; shapes: the (h, w) of every level of the memory; the first n_lvl are fused.
    -> (nchw [N, C, h0, w0] or None, cl [N, h0, w0, C] or None), or None when the library does not serve the shape (-2000): the caller
    keeps the torch composition."""
    if not (memory.is_cuda and memory.dtype == torch.float32 and memory.is_contiguous()):
        raise RuntimeError("memfuse: memory must be a contiguous fp32 GPU tensor: Not implemented on the CPU")
    shapes = tuple(tuple(int(v) for v in s) for s in shapes)
    try:
        return MemFuse.apply(memory, shapes, int(n_lvl), bool(want_nchw), bool(want_cl))
    except _NotServed:
        return None


class LsFeat(Function):
    @staticmethod
    def forward(ctx, lsf, txt, frames, b, t, size):
        nb, h, w, _ = lsf.shape
        (H, W), (Ho, Wo) = frames.shape[-2:], size
        tab_i, tab_w, off = ls_tables(h, w, H, W, Ho, Wo, lsf.device)
        out = torch.empty((b, t, 12, Ho, Wo), dtype=torch.float32, device=lsf.device)
        with torch.cuda.device(lsf.device):
            rc = lib().ocpg_lsfeat_fwd_f32(lsf.data_ptr(), _DT[lsf.dtype], txt.data_ptr(), frames.data_ptr(), tab_i.data_ptr(), tab_w.data_ptr(),
                                           off.data_ptr(), b, t, h, w, H, W, Ho, Wo, out.data_ptr(), stream_ptr())
        if rc == NOT_SERVED:
            raise _NotServed()
        check(rc, "ocpg_lsfeat_fwd_f32")
        ctx.save_for_backward(lsf, txt)
        ctx.meta = (b, t, H, W, Ho, Wo)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lsf, txt = ctx.saved_tensors
        b, t, H, W, Ho, Wo = ctx.meta
        nb, h, w, _ = lsf.shape
        g = g.float().contiguous()
        tab_i, tab_w, off = ls_tables(h, w, H, W, Ho, Wo, lsf.device)
        parts = lib().ocpg_lsfeat_bwd_parts(t, Ho, Wo)
        g_lsf = torch.empty(lsf.shape, dtype=torch.float32, device=lsf.device)
        part = torch.empty((b, parts, 8), dtype=torch.float32, device=lsf.device)
        with torch.cuda.device(lsf.device):
            check(lib().ocpg_lsfeat_bwd_f32(g.data_ptr(), lsf.data_ptr(), _DT[lsf.dtype], txt.data_ptr(), tab_i.data_ptr(), tab_w.data_ptr(),
                                            off.data_ptr(), b, t, h, w, Ho, Wo, g_lsf.data_ptr(), part.data_ptr(), stream_ptr()),
                  "ocpg_lsfeat_bwd_f32")
        return (g_lsf if lsf.dtype == torch.float32 else g_lsf.to(lsf.dtype)), part.sum(1), None, None, None, None


def lsfeat(lsf, txt, frames, b, t, size):
    """lsf [b*t, 8, h, w] (any strides; channels-last memory is read as it lies) in fp32 / bf16 / fp16, txt [b, 8], frames [b*t, 3, H, W];
    size = (Ho, Wo) -> ls_features [b, t, 12, Ho, Wo] fp32 (channels 0-2 the resized frames, 3-10 lsf, 11 sim), or None when the library
    does not serve the shape (-2000)."""
    if not (lsf.is_cuda and lsf.dtype in _DT and lsf.shape[1] == 8):
        raise RuntimeError("lsfeat: lsf must be a [N, 8, h, w] fp32 / bf16 / fp16 GPU tensor: Not implemented on the CPU")
    cl = lsf.permute(0, 2, 3, 1)
    cl = cl if cl.is_contiguous() else cl.contiguous()
    try:
        return LsFeat.apply(cl, txt.float().contiguous(), frames.float().contiguous(), int(b), int(t), (int(size[0]), int(size[1])))
    except _NotServed:
        return None
