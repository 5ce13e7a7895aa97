"""Inference tail of the mask output: binding of ocpg_mask_tail_f32 (csrc/mask_tail.hip).

The stride-4 mask logits go straight to what the drivers write (inference_davis.py:233-261, inference_ytvos.py): nearest x `up`,
un-pad crop, bilinear resize to the original size, sigmoid, then nothing (probabilities), `> threshold` (0 / on_value bytes) or the
multi-object merge (labels).  GPU tensors run the one HIP kernel; CPU tensors run the torch composition inference.py has always
used, so the host logic stays testable without a GPU.  No autograd: inference only.
"""
import torch
import torch.nn.functional as F

from ...._lib import check, lib, stream_ptr


def _launch(src, up, crop, out_size, mode, thr, bg, on_value, out):
    k, n, hs, ws = src.shape
    with torch.cuda.device(src.device):
        check(lib().ocpg_mask_tail_f32(src.data_ptr(), k, n, hs, ws, int(up), int(crop[0]), int(crop[1]), int(out_size[0]), int(out_size[1]),
                                       mode, float(thr), float(bg), int(on_value), out.data_ptr(), stream_ptr()), "ocpg_mask_tail_f32")
    return out


def _chain(src, up, crop, out_size):
    """The ATen chain: src [M, hs, ws] -> probabilities [M, out_h, out_w] fp32."""
    x = src.float()[None]
    if up != 1:
        x = F.interpolate(x, scale_factor=up)                                      # nearest, as the model's eval branch (ocpg.py:372)
    x = x[:, :, :crop[0], :crop[1]]                                                 # unpad (inference_davis.py:237)
    return F.interpolate(x, size=tuple(out_size), mode="bilinear", align_corners=False).sigmoid()[0]


def _check_geometry(src, up, crop, dims):
    if src.dim() != dims:
        raise ValueError(f"mask tail: expected a {dims}-d source, got {tuple(src.shape)}")
    hs, ws = src.shape[-2:]
    if not (1 <= crop[0] <= hs * up and 1 <= crop[1] <= ws * up):
        raise ValueError(f"mask tail: crop {tuple(crop)} outside the {hs * up} x {ws * up} map")


@torch.no_grad()
def mask_probabilities(src, up, crop, out_size):
    """src [N, hs, ws] logits -> fp32 [N, out_h, out_w] = sigmoid(bilinear(crop(nearest_up(src))))."""
    _check_geometry(src, up, crop, 3)
    if not src.is_cuda:
        return _chain(src, up, crop, out_size)
    src = src.float().contiguous()
    out = torch.empty((src.shape[0],) + tuple(out_size), dtype=torch.float32, device=src.device)
    return _launch(src[None], up, crop, out_size, 0, 0.0, 0.0, 0, out)


@torch.no_grad()
def mask_binary(src, up, crop, out_size, threshold=0.5, on_value=255):
    """src [N, hs, ws] logits -> uint8 [N, out_h, out_w]: on_value where the probability exceeds `threshold`, else 0."""
    _check_geometry(src, up, crop, 3)
    if not 0 <= int(on_value) <= 255:
        raise ValueError("mask_binary: on_value must fit a byte")
    if not src.is_cuda:
        return (_chain(src, up, crop, out_size) > threshold).to(torch.uint8).mul(int(on_value))
    src = src.float().contiguous()
    out = torch.empty((src.shape[0],) + tuple(out_size), dtype=torch.uint8, device=src.device)
    return _launch(src[None], up, crop, out_size, 1, threshold, 0.0, on_value, out)


@torch.no_grad()
def mask_labels(src, up, crop, out_size, threshold=0.3, background=0.1):
    """src [K, N, hs, ws] logits of K objects -> uint8 labels [N, out_h, out_w]: 0 = background, k + 1 = object k
    (inference_davis.py:253-261: probabilities below `threshold` zeroed, a constant `background` plane in front, first maximum)."""
    _check_geometry(src, up, crop, 4)
    k, n = src.shape[:2]
    if k > 255:
        raise ValueError("mask_labels: at most 255 objects fit a byte label")
    if not src.is_cuda:
        p = _chain(src.flatten(0, 1), up, crop, out_size).unflatten(0, (k, n))
        p[p < threshold] = 0.0
        return torch.cat([torch.full_like(p[:1], background), p], 0).argmax(0).to(torch.uint8)
    src = src.float().contiguous()
    out = torch.empty((n,) + tuple(out_size), dtype=torch.uint8, device=src.device)
    return _launch(src, up, crop, out_size, 2, threshold, background, 0, out)
