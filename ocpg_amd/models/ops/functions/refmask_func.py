"""A2D-Sentences / JHMDB-Sentences evaluation as integer counts: binding of ocpg_refmask_counts_f32 (csrc/refmask_counts.hip).

Per (sample, query) the three counts |P & G|, |P|, |G| from which P@K, overall IoU, mean IoU and the COCO AP figures follow
(ocpg_amd/metrics.py: RefMaskAccumulator, coco_ap_single_gt).  P is what A2DSentencesPostProcess (models/postprocessors.py) makes of
a query's mask logits: un-pad crop, bilinear resize to the original size, sigmoid, compare, invert; G is the sample's ground-truth
mask.  GPU tensors run the one HIP kernel, which decides every pixel from the low-resolution source and writes nothing at the original
resolution; CPU tensors run the post-processor's chain as a torch composition, so the host logic stays testable without a GPU.
"""
import torch
import torch.nn.functional as F

from ...._lib import check, lib, stream_ptr

GT_ALIGN = 4          # each ground-truth plane starts on a 4-byte boundary of the packed buffer: whole-word loads on every row


def _pairs(x, name, n):
    x = x.tolist() if torch.is_tensor(x) else [tuple(int(v) for v in p) for p in x]
    if len(x) != n or any(len(p) != 2 for p in x):
        raise ValueError(f"refmask_counts: {name} must hold one (h, w) per sample")
    return [(int(p[0]), int(p[1])) for p in x]


def _composition(src, up, crops, out_sizes, gt_masks, threshold, invert):
    out = torch.empty((src.shape[0], src.shape[1], 3), dtype=torch.int64, device=src.device)
    for b, (m, (ch, cw), size, g) in enumerate(zip(src, crops, out_sizes, gt_masks)):
        if up != 1:
            m = F.interpolate(m[None], scale_factor=up)[0]                              # nearest, as the model's eval branch
        m = F.interpolate(m[:, :ch, :cw].unsqueeze(1).float(), size=size, mode="bilinear", align_corners=False)
        p = m.sigmoid() > threshold
        p = ~p if invert else p                                                         # [q, 1, H0, W0] bool
        g = (g != 0).to(src.device)[None, None]
        out[b, :, 0] = (p & g).flatten(1).sum(1)
        out[b, :, 1] = p.flatten(1).sum(1)
        out[b, :, 2] = g.sum()
    return out


def pack_gt(gt_masks, device):
    """[H0, W0] bool / uint8 masks -> (uint8 buffer on `device`, int64 start offsets on the host), one row-major plane per sample,
    each starting on a GT_ALIGN boundary; the gaps are never read."""
    offs, total = [], 0
    for g in gt_masks:
        offs.append(total)
        total += (g.numel() + GT_ALIGN - 1) // GT_ALIGN * GT_ALIGN
    buf = torch.empty(max(total, GT_ALIGN), dtype=torch.uint8, device=device)
    for g, o in zip(gt_masks, offs):
        buf[o:o + g.numel()].view(g.shape).copy_(g if g.dtype == torch.uint8 else g != 0)
    return buf, torch.tensor(offs, dtype=torch.int64)


@torch.no_grad()
def refmask_counts(src, up, crops, out_sizes, gt_masks, threshold=0.5, invert=True, native=None):
    """src fp32 logits [B, Q, hs, ws] -> int64 [B, Q, 3] = (|P & G|, |P|, |G|) per sample and query.

    up: nearest replication factor of src (1 for `pred_masks` as forward returns them, 4 for `pred_masks_low`).  crops / out_sizes: one
    (h, w) per sample (lists or [B, 2] tensors): the un-padded augmented size, at most (hs * up, ws * up), and the original size.
    gt_masks: a list of [H0, W0] bool / uint8 tensors, H0, W0 = the sample's out size.  invert: the reference's `1 - (sigmoid > 0.5)`.
    native: None = the kernel for GPU tensors, the torch composition for CPU tensors; True = the kernel or an error; False = the
    composition (tools/refmask_ab.py times one against the other).
    """
    if src.dim() != 4 or not src.dtype.is_floating_point:
        raise ValueError(f"refmask_counts: expected floating-point logits [B, Q, hs, ws], got {tuple(src.shape)} {src.dtype}")
    b, q, hs, ws = src.shape
    up = int(up)
    if min(b, q, hs, ws) < 1 or up < 1:
        raise ValueError("refmask_counts: empty logits or up < 1")
    crops, out_sizes = _pairs(crops, "crops", b), _pairs(out_sizes, "out_sizes", b)
    if len(gt_masks) != b:
        raise ValueError("refmask_counts: one ground-truth mask per sample")
    for (ch, cw), (oh, ow), g in zip(crops, out_sizes, gt_masks):
        if not (1 <= ch <= hs * up and 1 <= cw <= ws * up):
            raise ValueError(f"refmask_counts: crop {(ch, cw)} outside the {hs * up} x {ws * up} map")
        if oh < 1 or ow < 1 or oh * ow >= 1 << 31:
            raise ValueError(f"refmask_counts: original size {(oh, ow)} not served")
        if tuple(g.shape) != (oh, ow) or g.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"refmask_counts: ground truth {tuple(g.shape)} {g.dtype} is not a bool / uint8 mask of size {(oh, ow)}")
    if native is None:
        native = src.is_cuda
    if not native:
        return _composition(src, up, crops, out_sizes, gt_masks, float(threshold), bool(invert))
    if not src.is_cuda:
        raise RuntimeError("refmask_counts: the kernel needs GPU tensors")
    src = src.float().contiguous()
    gt, off_host = pack_gt(gt_masks, src.device)
    # both tables in one upload: [B] int64 offsets, then [B, 4] int32 geometry (8-byte aligned behind them)
    table = torch.empty(3 * b, dtype=torch.int64)
    table[:b] = off_host
    table[b:].view(torch.int32).view(b, 4).copy_(torch.tensor([c + o for c, o in zip(crops, out_sizes)], dtype=torch.int32))
    table_dev = table.to(src.device)
    out = torch.empty((b, q, 3), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        check(lib().ocpg_refmask_counts_f32(src.data_ptr(), b, q, hs, ws, up, table.data_ptr() + 8 * b, table_dev.data_ptr() + 8 * b,
                                            gt.data_ptr(), table_dev.data_ptr(), max(o[0] for o in out_sizes), max(o[1] for o in out_sizes),
                                            float(threshold), int(bool(invert)), out.data_ptr(), stream_ptr()),
              "ocpg_refmask_counts_f32")
    return out.to(torch.int64)
