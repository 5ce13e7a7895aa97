"""Similarity head of the weak-annotation generator: binding of ocpg_sim_heat_f32 (csrc/sim_heat.hip).

Per object o on frame f with candidate feature cells c (reference pre_process/sim_model.py:35-134), k^_p = feat[f, p] / |feat[f, p]|:
    a_c[p] = k^_c . k^_p,   s_c[p] = (a_c[p] - min_p a_c) / max_p a_c       (divided by the maximum, as the reference has it)
point mode (box None): heat[o] = s of the object's one candidate.  Box mode: every candidate is scored by the soft IoU of the row /
column maxima of s_c with the box's projections, the best one (lowest index among equals) gives the plane.  An object without
candidates gets a zero plane and choice -1.

GPU tensors within the kernel's served range run the HIP kernel; CPU tensors, shapes outside the range and native=False run a
batched torch composition of the same definition (one matrix product per frame, no per-candidate loop), so the host logic stays
testable without a GPU.  tools/sim_heat_ab.py times one against the other: the kernel beat the composition 3.1x and 4.0x at the two
measured shapes with identical runs within 7-9 % (profiles/sim_heat_ab.jsonl), so it is the default on the GPU.
"""
import ctypes

import torch

from ...._lib import check, lib, stream_ptr

MAX_CANDIDATES = 256
MAX_PIXELS = 8192


def served(feat, counts):
    """The kernel's range: C % 4 == 0, h*w <= 8192, at most 256 candidates per object, 16-byte aligned features."""
    f, h, w, c = feat.shape
    return (c % 4 == 0 and h * w <= MAX_PIXELS and f * h * w < 2 ** 31 and 1 <= len(counts) <= 65535
            and (not counts or max(counts) <= MAX_CANDIDATES))


def _composition(feat, obj_frame, cand_off, cand_xy, box):
    f, h, w, c = feat.shape
    p = h * w
    dev = feat.device
    n_obj = obj_frame.numel()
    off = cand_off.to(dev, torch.int64)
    counts = off[1:] - off[:-1]
    total = int(off[-1])
    heat = torch.zeros((n_obj, p), dtype=torch.float32, device=dev)
    choice = torch.full((n_obj,), -1, dtype=torch.int32, device=dev)
    score = torch.zeros((total,), dtype=torch.float32, device=dev)
    if total == 0:
        return heat.view(n_obj, h, w), choice, score
    khat = feat.reshape(f, p, c)
    khat = khat / khat.norm(dim=-1, keepdim=True)
    obj_of = torch.repeat_interleave(torch.arange(n_obj, device=dev), counts)
    frame_of = obj_frame.to(dev, torch.int64)[obj_of]
    xy = cand_xy.to(dev, torch.int64)
    q = khat[frame_of, xy[:, 1] * w + xy[:, 0]]                                        # [total, C]
    a = torch.empty((total, p), dtype=torch.float32, device=dev)
    for fr in torch.unique(frame_of).tolist():                                           # one product per frame that has candidates
        idx = torch.nonzero(frame_of == fr)[:, 0]
        a[idx] = q[idx] @ khat[fr].t()
    s = (a - a.amin(1, keepdim=True)) / a.amax(1, keepdim=True)
    has = counts > 0
    if box is None:
        best = torch.zeros((n_obj,), dtype=torch.int64, device=dev)
    else:
        planes = s.view(total, h, w)
        b = box.to(dev, torch.int64)[obj_of]
        xs, ys = torch.arange(w, device=dev)[None], torch.arange(h, device=dev)[None]
        bx = ((xs >= b[:, 0:1]) & (xs < b[:, 2:3])).to(torch.float32)
        by = ((ys >= b[:, 1:2]) & (ys < b[:, 3:4])).to(torch.float32)
        mx, my = planes.amax(1), planes.amax(2)
        score = 0.5 * ((mx * bx).sum(1) / ((mx + bx - mx * bx).sum(1) + 1e-5) + (my * by).sum(1) / ((my + by - my * by).sum(1) + 1e-5))
        # best candidate per object, the lowest index among equal scores: arg-max rules differ between devices, this does not
        pos = torch.arange(total, device=dev) - off[:-1][obj_of]
        width = int(counts.max())
        table = torch.full((n_obj, width), float("-inf"), dtype=torch.float32, device=dev)
        table[obj_of, pos] = score
        top = table.amax(1, keepdim=True)
        best = torch.where(table == top, torch.arange(width, device=dev)[None], width).amin(1).clamp(max=width - 1)
    sel = (off[:-1] + best)[has]
    heat[has] = s[sel]
    choice[has] = best[has].to(torch.int32)
    return heat.view(n_obj, h, w), choice, score


@torch.no_grad()
def sim_heat(feat, obj_frame, cand_off, cand_xy, box=None, native=None):
    """feat fp32 [F, h, w, C] (channels last) -> (heat fp32 [n_obj, h, w], choice int32 [n_obj], score fp32 [total]).

    obj_frame int [n_obj]: the frame of each object.  cand_off int [n_obj + 1], starting at 0 and ascending: object o owns the rows
    cand_off[o] .. cand_off[o+1]-1 of cand_xy int [total, 2] ((x, y) feature cells).  box int [n_obj, 4] ((x0, y0, x1, y1) feature cells,
    ends exclusive) or None for point mode (choice 0, score 0).  native: None = the kernel for GPU tensors within its served
    range, the torch composition otherwise; True = the kernel or an error; False = the composition.
    """
    if feat.dim() != 4 or feat.dtype != torch.float32:
        raise ValueError(f"sim_heat: feat must be fp32 [F, h, w, C], got {feat.dtype} {tuple(feat.shape)}")
    f, h, w, c = feat.shape
    offs = [int(v) for v in cand_off.tolist()]
    n_obj = obj_frame.numel()
    if len(offs) != n_obj + 1 or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("sim_heat: cand_off must hold n_obj + 1 ascending offsets starting at 0")
    total = offs[-1]
    if tuple(cand_xy.shape) != (total, 2):
        raise ValueError(f"sim_heat: cand_xy must be [{total}, 2], got {tuple(cand_xy.shape)}")
    if box is not None and tuple(box.shape) != (n_obj, 4):
        raise ValueError(f"sim_heat: box must be [{n_obj}, 4], got {tuple(box.shape)}")
    if min(f, h, w, c) < 1:
        raise ValueError("sim_heat: empty features")
    frames = obj_frame.tolist()
    if frames and not (0 <= min(frames) and max(frames) < f):
        raise ValueError("sim_heat: obj_frame outside the features")
    if total:
        lo, hi = cand_xy.amin(0).tolist(), cand_xy.amax(0).tolist()
        if lo[0] < 0 or lo[1] < 0 or hi[0] >= w or hi[1] >= h:
            raise ValueError("sim_heat: candidate cell outside the feature map")
    counts = [b - a for a, b in zip(offs, offs[1:])]
    if n_obj == 0:
        return (torch.zeros((0, h, w), dtype=torch.float32, device=feat.device), torch.zeros((0,), dtype=torch.int32, device=feat.device),
                torch.zeros((0,), dtype=torch.float32, device=feat.device))
    ok = feat.is_cuda and served(feat, counts)
    if native is None:
        native = ok
    if not native:
        return _composition(feat, obj_frame, torch.as_tensor(offs), cand_xy, box)
    if not feat.is_cuda:
        raise RuntimeError("sim_heat: the kernel needs GPU tensors")
    if not ok:
        raise RuntimeError("sim_heat: outside the kernel's served range (C % 4 == 0, h*w <= 8192, at most 256 candidates per object)")
    dev = feat.device
    feat = feat.contiguous()
    if feat.data_ptr() % 16:
        feat = feat.clone()
    i32 = dict(dtype=torch.int32, device=dev)
    obj_frame_d = obj_frame.to(**i32).contiguous()
    off_host = (ctypes.c_int * (n_obj + 1))(*offs)
    off_d = torch.tensor(offs, **i32)
    xy_d = cand_xy.to(**i32).contiguous()
    box_d = None if box is None else box.to(**i32).contiguous()
    heat = torch.empty((n_obj, h, w), dtype=torch.float32, device=dev)
    choice = torch.empty((n_obj,), dtype=torch.int32, device=dev)
    score = torch.empty((total,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L = lib()
        work = torch.empty((int(L.ocpg_sim_heat_workspace(f, h, w, total)) // 4 + 4,), dtype=torch.float32, device=dev)
        check(L.ocpg_sim_heat_f32(feat.data_ptr(), f, h, w, c, n_obj, obj_frame_d.data_ptr(), ctypes.addressof(off_host), off_d.data_ptr(),
                                  xy_d.data_ptr(), None if box_d is None else box_d.data_ptr(), heat.data_ptr(), choice.data_ptr(),
                                  score.data_ptr(), work.data_ptr(), stream_ptr()),
              "ocpg_sim_heat_f32")
    return heat, choice, score
