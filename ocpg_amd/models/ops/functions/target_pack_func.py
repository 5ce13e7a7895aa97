"""The target pack: every tensor the matcher and the criterion derive from the batch's targets alone -- the /32-padded ground truth
sub-sampled at the criterion's and the matcher's strides, the rasterised boxes (full, low and level-set resolution), the weak masks
inside the box, the heat-map weights of the masked BCE, and the [B, T] stacks of boxes / valid / labels (reference
models/criterion.py:109-190, models/matcher.py:100-114, models/segmentation.py:177-190).

`build_target_pack(..., native=True)` is csrc/target_pack.hip: ceil(B/16) + 1 launches, the clips' pointers passed by value (no
host-to-device copy: capturable).  `native=False` is the torch composition the matcher and the criterion ran before (about a hundred
tiny ATen kernels) -- the reference the kernel is tested against bit for bit, the CPU path, and the path of shapes the kernel
does not serve.  The pack is built from one `targets` list and lives for one forward: nothing is cached across calls.
"""
import ctypes
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from ....util import box_ops
from ....util.misc import nested_tensor_from_tensor_list

NATIVE = os.environ.get("OCPG_TARGET_PACK", "1") != "0"      # A/B switch, read once at import

CRITERION_KEYS = ("masks", "weights", "weak_masks", "boxes", "valid", "size")


def _pad_stack(targets, key):
    return nested_tensor_from_tensor_list([t[key] for t in targets], size_divisibility=32, split=False).decompose()[0]


def _sub(x, k):
    return x[..., k // 2::k, k // 2::k]


def heat_weight(h, reg):
    """masked_ce_loss's weight map (segmentation.py:177-190): targets only."""
    w = (h.clamp(min=0.3, max=0.7) - 0.5).abs()
    lo, hi = w.min(), w.max()
    w = (w - lo) / (hi - lo + 1e-5)
    return torch.where(reg == 0, torch.ones_like(w), w)


def matcher_targets(targets, sm, labels=True):
    """The matcher's share alone: (gt_m [B,T,PH/sm,PW/sm] fp32, valid_f [B,T] fp32, tboxes [B,T,4] fp32, labels [B,T] int64 or None)."""
    gt, _ = nested_tensor_from_tensor_list([t["masks"] for t in targets], size_divisibility=32, split=False).decompose()
    gt = gt.to(torch.float32)
    im_h, im_w = gt.shape[-2:]
    gt = gt[:, :, sm // 2::sm, sm // 2::sm]
    assert gt.size(2) * sm == im_h and gt.size(3) * sm == im_w
    valid = torch.stack([t["valid"] for t in targets]).to(torch.float32)                                 # [B, T]
    tb = torch.stack([t["boxes"] for t in targets]).to(torch.float32)                                    # [B, T, 4]
    lab = torch.stack([t["labels"] for t in targets]).to(torch.int64) if labels and "labels" in targets[0] else None
    return gt, valid, tb, lab


def _compose(targets, s, sl, sm, ls_hw):
    from ...segmentation import generate_box_region_mask
    gt = _pad_stack(targets, "masks").to(torch.float32)
    heat = _pad_stack(targets, "weights").to(torch.float32)
    weak = _pad_stack(targets, "weak_masks").to(torch.float32)
    im_h, im_w = gt.shape[-2:]
    b, nf = weak.shape[:2]
    gt_full = _sub(gt, s)
    assert gt_full.size(2) * s == im_h and gt_full.size(3) * s == im_w
    sizes = torch.stack([t["size"] for t in targets]).repeat_interleave(nf, dim=0)
    boxes = box_ops.box_cxcywh_to_xyxy(torch.cat([t["boxes"] for t in targets], dim=0))
    region = generate_box_region_mask(boxes, (im_h, im_w), sizes).view(b, nf, im_h, im_w)
    region_low, region = _sub(region, sl), _sub(region, s)
    weak_full, weak_low = _sub(weak, s) * region, _sub(weak, sl) * region_low
    w_full, w_low = heat_weight(_sub(heat, s), region), heat_weight(_sub(heat, sl), region_low)
    region_scaled = F.interpolate(region, tuple(ls_hw), mode="nearest").flatten(0, 1)
    gt_m, valid_f, tboxes, labels = matcher_targets(targets, sm)
    return SimpleNamespace(gt_s=gt_full, gt_m=gt_m, region_s=region, region_l=region_low, region_ls=region_scaled, weak_s=weak_full,
                           weak_l=weak_low, w_s=w_full, w_l=w_low, tboxes=tboxes, valid_f=valid_f,
                           valid_i=torch.stack([t["valid"] for t in targets]), labels=labels)


def _ceil32(v):
    return (v + 31) // 32 * 32


def _native(targets, s, sl, sm, ls_hw):
    """-> the pack, or None where the kernel does not serve the shape (-2000)."""
    from ...._lib import check, lib
    b = len(targets)
    dev = targets[0]["masks"].device
    keep = []       # the fp32 / int64 / dense forms the pointers below address (alive until the launches are enqueued)

    def ptrs(key, dtype):
        ts = [t[key].to(dtype).contiguous() for t in targets]
        keep.append(ts)
        return (ctypes.c_void_p * b)(*[x.data_ptr() for x in ts]), ts

    masks, m = ptrs("masks", torch.float32)
    heat, h = ptrs("weights", torch.float32)
    weak, w = ptrs("weak_masks", torch.float32)
    nf = m[0].shape[0]
    for i in range(b):
        assert m[i].ndim == 3 and m[i].shape == h[i].shape == w[i].shape and m[i].shape[0] == nf, "masks / weights / weak_masks disagree"
        assert targets[i]["boxes"].shape == (nf, 4) and targets[i]["valid"].shape == (nf,) and targets[i]["size"].shape == (2,)
    boxes, _ = ptrs("boxes", torch.float32)
    valid, _ = ptrs("valid", torch.int64)
    size, _ = ptrs("size", torch.int64)
    labels = None
    if "labels" in targets[0]:
        labels, lab = ptrs("labels", torch.int64)
        assert all(x.shape == (nf,) for x in lab)
    hw = (ctypes.c_int * (2 * b))(*[v for x in m for v in x.shape[1:]])
    ph, pw = _ceil32(max(x.shape[1] for x in m)), _ceil32(max(x.shape[2] for x in m))
    lh, lw = int(ls_hw[0]), int(ls_hw[1])

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    p = SimpleNamespace(gt_s=f32(b, nf, ph // s, pw // s), gt_m=f32(b, nf, ph // sm, pw // sm), region_s=f32(b, nf, ph // s, pw // s),
                        region_l=f32(b, nf, ph // sl, pw // sl), region_ls=f32(b * nf, lh, lw), weak_s=f32(b, nf, ph // s, pw // s),
                        weak_l=f32(b, nf, ph // sl, pw // sl), w_s=f32(b, nf, ph // s, pw // s), w_l=f32(b, nf, ph // sl, pw // sl),
                        tboxes=f32(b, nf, 4), valid_f=f32(b, nf), valid_i=torch.empty((b, nf), dtype=torch.int64, device=dev),
                        labels=None if labels is None else torch.empty((b, nf), dtype=torch.int64, device=dev))
    ws = torch.empty((max(int(lib().ocpg_target_pack_workspace(b)), 16),), dtype=torch.uint8, device=dev)
    rc = lib().ocpg_target_pack_f32(b, nf, masks, heat, weak, hw, boxes, valid, labels, size, ph, pw, s, sl, sm, lh, lw, p.gt_s.data_ptr(),
                                    p.gt_m.data_ptr(), p.region_s.data_ptr(), p.region_l.data_ptr(), p.region_ls.data_ptr(),
                                    p.weak_s.data_ptr(), p.weak_l.data_ptr(), p.w_s.data_ptr(), p.w_l.data_ptr(), p.tboxes.data_ptr(),
                                    p.valid_f.data_ptr(), p.valid_i.data_ptr(), None if p.labels is None else p.labels.data_ptr(),
                                    ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc == -2000:
        return None
    check(rc, "ocpg_target_pack_f32")
    return p


def build_target_pack(targets, s, sl, sm, ls_hw, native=None):
    """targets: the batch's list of dicts (CRITERION_KEYS, optionally 'labels'); s, sl: the criterion's mask strides, sm: the
    matcher's; ls_hw: the level-set map size.  -> SimpleNamespace(gt_s, gt_m, region_s, region_l, region_ls, weak_s, weak_l, w_s, w_l,
    tboxes, valid_f, valid_i, labels, targets, key); `targets` is the very list it was built from and `key` = (s, sl, sm, ls_hw): a
    consumer uses the pack only where both are its own."""
    if native is None:
        native = NATIVE
    ls_hw = (int(ls_hw[0]), int(ls_hw[1]))
    p = None
    if native and targets[0]["masks"].is_cuda:
        p = _native(targets, s, sl, sm, ls_hw)
    if p is None:
        with torch.no_grad(), torch.autocast(device_type=targets[0]["masks"].device.type, enabled=False):
            p = _compose(targets, s, sl, sm, ls_hw)
    p.targets, p.key = targets, (s, sl, sm, ls_hw)
    return p
