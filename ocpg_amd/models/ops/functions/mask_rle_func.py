"""COCO run-length encoding on the device: binding of csrc/mask_rle.hip (ocpg_mask_rle_query / ocpg_mask_rle_pack_u8 /
ocpg_mask_rle_pack_logits_f32 / ocpg_mask_rle_encode).

`rle_encode_masks` takes boolean planes, `rle_from_logits` the mask logits themselves (the post-processor's chain -- un-pad crop,
bilinear resize to the original size, sigmoid, compare, invert -- is decided per pixel inside the kernel, as in refmask_func).  Both
return the dicts models/postprocessors.py: rle_encode returns, byte for byte.  GPU tensors run the kernels: the planes never reach
the host, only the transition totals (to size the counts) and the strings do.  CPU tensors run the host loop, so the logic stays
testable without a GPU.  The number of runs depends on the data, so a call synchronises twice and cannot be captured.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ...._lib import check, lib, stream_ptr
from .refmask_func import _pairs


def counts_to_string(counts) -> bytes:
    """Run lengths -> the compressed COCO string, vectorised over the counts (what the kernel's third pass computes per run):
    x = c[i] - c[i-2] from the fourth count on, 5-bit groups low first, 0x20 = another group follows, + 48."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    x = c.copy()
    x[3:] -= c[1:-2]
    groups = [(x >> (5 * k)) & 0x1F for k in range(8)]                    # arithmetic shifts: 2's complement of any |x| < 2^39
    rest = [x >> (5 * (k + 1)) for k in range(8)]
    last = [np.where(g & 0x10, r == -1, r == 0) for g, r in zip(groups, rest)]
    n = np.argmax(np.stack(last, 1), 1) + 1 if len(x) else np.zeros(0, dtype=np.int64)       # characters per count: the first last group
    out = np.zeros((len(x), 8), dtype=np.uint8)
    for k in range(8):
        out[:, k] = groups[k] + 48 + np.where(k + 1 < n, 0x20, 0)
    return out[np.arange(8)[None, :] < n[:, None]].tobytes()


def string_to_counts(data) -> list:
    """The compressed COCO string -> run lengths (the first half of postprocessors.rle_decode)."""
    data = data.encode() if isinstance(data, str) else bytes(data)
    counts, p = [], 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            ch = data[p] - 48
            x |= (ch & 0x1F) << (5 * k)
            more = bool(ch & 0x20)
            p += 1
            k += 1
            if not more and (ch & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_area(rle) -> int:
    """Set pixels of an encoded mask: the sum of its odd runs."""
    return int(sum(string_to_counts(rle["counts"])[1::2]))


def workspace_bytes(n_masks, max_n, what="workspace") -> int:
    """Bytes of device workspace for n_masks masks of at most max_n pixels (ocpg_mask_rle_query; what="chunk": the chunk size)."""
    import ctypes
    size, chunk = ctypes.c_longlong(0), ctypes.c_int(0)
    check(lib().ocpg_mask_rle_query(int(n_masks), int(max_n), ctypes.addressof(size), ctypes.addressof(chunk), None), "ocpg_mask_rle_query")
    return int(chunk.value if what == "chunk" else size.value)


def chunk_pixels() -> int:
    """Pixels of the column-major order one workgroup of the first two passes owns."""
    return workspace_bytes(1, 1, "chunk")


def _encode(device, sizes, pack):
    """Steps 1 and 2 around the one readback that sizes the counts.  sizes: (h, w) per mask; pack(max_n, n_trans, workspace)
    launches the first pass.  -> list of dicts."""
    n = len(sizes)
    max_n = max(h * w for h, w in sizes)
    L = lib()
    ws_bytes = workspace_bytes(n, max_n)
    with torch.cuda.device(device):
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        n_trans = torch.empty(n, dtype=torch.int32, device=device)
        pack(max_n, n_trans, workspace)
        n_trans_host = n_trans.cpu()                                                      # readback 1: [n] totals
        start = torch.zeros(n, dtype=torch.int64)
        start[1:] = torch.cumsum(n_trans_host[:-1].long() + 1, 0)
        cap = int(start[-1]) + int(n_trans_host[-1]) + 1
        start_dev = start.to(device)
        counts = torch.empty(cap, dtype=torch.int32, device=device)
        n_runs = torch.empty(n, dtype=torch.int32, device=device)
        out = torch.empty(8 * n + 7 * cap, dtype=torch.uint8, device=device)              # [n] int64 string lengths, then the strings
        check(L.ocpg_mask_rle_encode(n, max_n, n_trans_host.data_ptr(), start.data_ptr(), start_dev.data_ptr(), cap, counts.data_ptr(),
                                     n_runs.data_ptr(), out.data_ptr() + 8 * n, out.data_ptr(), workspace.data_ptr(), stream_ptr()),
              "ocpg_mask_rle_encode")
        host = out.cpu().numpy()                                                          # readback 2: lengths and strings together
    n_bytes = host[:8 * n].view(np.int64)
    text = host[8 * n:]
    return [{"size": [int(h), int(w)], "counts": text[7 * s:7 * s + int(nb)].tobytes()}
            for (h, w), s, nb in zip(sizes, start.tolist(), n_bytes)]


@torch.no_grad()
def rle_encode_masks(masks, native=None):
    """A list of [H, W] bool / uint8 planes (sizes may differ), or one [n, H, W] tensor -> [{"size": [h, w], "counts": bytes}].
    Non-zero = set.  native: None = the kernels for GPU tensors, the host loop for CPU tensors; True = the kernels or an error; False =
    the host loop (postprocessors.rle_encode)."""
    planes = list(masks)
    for p in planes:
        if not torch.is_tensor(p) or p.dim() != 2 or p.dtype not in (torch.bool, torch.uint8):
            raise ValueError("rle_encode_masks: expected [H, W] bool / uint8 planes")
    if not planes:
        return []
    on_gpu = all(p.is_cuda for p in planes)
    if native is None:
        native = on_gpu
    if not native:
        from ...postprocessors import rle_encode
        return [rle_encode(p if p.dtype == torch.bool else p != 0) for p in planes]       # non-zero = set, as the kernel reads it
    if not on_gpu or len({p.device for p in planes}) != 1:
        raise RuntimeError("rle_encode_masks: the kernel needs GPU tensors on one device")
    if any(p.numel() == 0 or p.numel() >= 1 << 31 for p in planes):
        raise ValueError("rle_encode_masks: an empty plane or one of 2^31 pixels or more is not served")
    planes = [p.contiguous() for p in planes]                                             # row-major planes; kept alive over the call
    sizes = [(int(p.shape[0]), int(p.shape[1])) for p in planes]
    n, device = len(planes), planes[0].device
    base = min(p.data_ptr() for p in planes)
    # both tables in one upload: [n] int64 byte offsets from the lowest plane, then [n, 2] int32 geometry
    table = torch.empty(2 * n, dtype=torch.int64)
    table[:n] = torch.tensor([p.data_ptr() - base for p in planes], dtype=torch.int64)
    table[n:].view(torch.int32).view(n, 2).copy_(torch.tensor(sizes, dtype=torch.int32))
    table_dev = table.to(device)

    def pack(max_n, n_trans, workspace):
        check(lib().ocpg_mask_rle_pack_u8(base, table_dev.data_ptr(), n, table.data_ptr() + 8 * n, table_dev.data_ptr() + 8 * n, max_n,
                                          n_trans.data_ptr(), workspace.data_ptr(), stream_ptr()), "ocpg_mask_rle_pack_u8")
    return _encode(device, sizes, pack)


def _chain(src, up, crops, out_sizes, threshold, invert):
    """The post-processor's chain as a torch composition (refmask_func._composition without the counting) -> per sample [Q, H0, W0]."""
    out = []
    for m, (ch, cw), size in zip(src, crops, out_sizes):
        if up != 1:
            m = F.interpolate(m[None], scale_factor=up)[0]
        m = F.interpolate(m[:, :ch, :cw].unsqueeze(1).float(), size=size, mode="bilinear", align_corners=False)
        p = m.sigmoid() > threshold
        out.append((~p if invert else p)[:, 0])
    return out


@torch.no_grad()
def rle_from_logits(src, up, crops, out_sizes, threshold=0.5, invert=True, native=None):
    """src fp32 logits [B, Q, hs, ws] -> [B][Q] dicts {"size": [h, w], "counts": bytes}: every query's mask at the original size,
    run-length encoded.  up, crops, out_sizes, threshold, invert as refmask_func.refmask_counts.  native: None = the kernels for GPU
    tensors, the torch chain and the host loop for CPU tensors; True = the kernels or an error; False = chain and host loop."""
    if src.dim() != 4 or not src.dtype.is_floating_point:
        raise ValueError(f"rle_from_logits: expected floating-point logits [B, Q, hs, ws], got {tuple(src.shape)} {src.dtype}")
    b, q, hs, ws = src.shape
    up = int(up)
    if min(b, q, hs, ws) < 1 or up < 1:
        raise ValueError("rle_from_logits: empty logits or up < 1")
    crops, out_sizes = _pairs(crops, "crops", b), _pairs(out_sizes, "out_sizes", b)
    for (ch, cw), (oh, ow) in zip(crops, out_sizes):
        if not (1 <= ch <= hs * up and 1 <= cw <= ws * up):
            raise ValueError(f"rle_from_logits: crop {(ch, cw)} outside the {hs * up} x {ws * up} map")
        if oh < 1 or ow < 1 or oh * ow >= 1 << 31:
            raise ValueError(f"rle_from_logits: original size {(oh, ow)} not served")
    if native is None:
        native = src.is_cuda
    if not native:
        from ...postprocessors import rle_encode
        return [[rle_encode(p) for p in planes.cpu()] for planes in _chain(src, up, crops, out_sizes, float(threshold), bool(invert))]
    if not src.is_cuda:
        raise RuntimeError("rle_from_logits: the kernel needs GPU tensors")
    src = src.float().contiguous()
    geom = torch.tensor([c + o for c, o in zip(crops, out_sizes)], dtype=torch.int32)
    geom_dev = geom.to(src.device)

    def pack(max_n, n_trans, workspace):
        check(lib().ocpg_mask_rle_pack_logits_f32(src.data_ptr(), b, q, hs, ws, up, geom.data_ptr(), geom_dev.data_ptr(), max_n,
                                                  float(threshold), int(bool(invert)), n_trans.data_ptr(), workspace.data_ptr(),
                                                  stream_ptr()), "ocpg_mask_rle_pack_logits_f32")
    flat = _encode(src.device, [o for o in out_sizes for _ in range(q)], pack)
    return [flat[i * q:(i + 1) * q] for i in range(b)]
