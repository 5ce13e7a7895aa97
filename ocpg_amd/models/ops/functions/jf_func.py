"""DAVIS-2017 J&F scoring as integer counts: binding of ocpg_jf_counts_u8 (csrc/jf_metrics.hip).

Per (result id, ground-truth id) pair and frame the six counts from which region similarity J and boundary accuracy F follow
(reference davis2017/metrics.py: db_eval_iou, f_measure, _seg2bmap): |A&B|, |A|B|, |b(A)|, |b(B)|, matched pixels of b(A), matched
pixels of b(B).  GPU tensors run the one HIP kernel; CPU tensors run a torch composition (shifts for the boundary map, conv2d with the
disk for the dilation), so the host logic stays testable without a GPU.  A radius above the kernel's served range runs the same
composition on the device.  ocpg_amd.metrics.jf_from_counts turns the counts into J and F.
"""
import torch
import torch.nn.functional as F

from ...._lib import check, lib, stream_ptr

MAX_KERNEL_RADIUS = 64
MAX_IDS = 254


def boundary_map(m):
    """m [..., H, W] bool -> the reference's _seg2bmap at equal size (neighbours outside the image count as 0)."""
    e = F.pad(m[..., :, 1:], (0, 1))
    s = F.pad(m[..., 1:, :], (0, 0, 0, 1))
    se = F.pad(m[..., 1:, 1:], (0, 1, 0, 1))
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[..., -1, :] = m[..., -1, :] ^ e[..., -1, :]
    b[..., :, -1] = m[..., :, -1] ^ s[..., :, -1]
    b[..., -1, -1] = False
    return b


def disk(radius, device=None):
    """skimage.morphology.disk: [2r+1, 2r+1] fp32, 1 where dx^2 + dy^2 <= r^2."""
    a = torch.arange(-radius, radius + 1, device=device)
    return ((a[:, None] ** 2 + a[None, :] ** 2) <= radius * radius).to(torch.float32)


def _dilate(b, k):
    """b [N, H, W] bool, k the disk -> bool: a set pixel within the disk; pixels outside the image never win (zero padding)."""
    r = k.shape[0] // 2
    return F.conv2d(b[:, None].to(torch.float32), k[None, None], padding=r)[:, 0] > 0.5      # sums of 0/1: exact in fp32


def _composition(gt, res, num_gt, num_res, radius, void_label, all_pairs):
    t = gt.shape[0]
    keep = gt != void_label if void_label is not None else torch.ones_like(gt, dtype=torch.bool)
    k = disk(radius, gt.device)
    n_res = num_res if all_pairs else num_gt

    def side(labels, n):
        m = [(labels == i + 1) & keep for i in range(n)]
        b = [boundary_map(x) for x in m]
        return m, b, [_dilate(x, k) for x in b]

    ma, ba, da = side(res, n_res)
    mb, bb, db = side(gt, num_gt)
    pairs = [(r, g) for r in range(n_res) for g in range(num_gt)] if all_pairs else [(g, g) for g in range(num_gt)]
    out = torch.empty((len(pairs), t, 6), dtype=torch.int32, device=gt.device)
    for p, (r, g) in enumerate(pairs):
        for i, x in enumerate((ma[r] & mb[g], ma[r] | mb[g], ba[r], bb[g], ba[r] & db[g], bb[g] & da[r])):
            out[p, :, i] = x.flatten(1).sum(1)
    return out


@torch.no_grad()
def jf_counts(gt, res, num_gt, num_res=None, radius=None, void_label=None, all_pairs=False, native=None):
    """gt, res uint8 label maps [T, H, W] (0 = background, k = object / proposal k) -> int32 [P, T, 6].

    all_pairs False: P = num_gt, pair p = (result id p+1, gt id p+1).  True: P = num_res * num_gt, pair r * num_gt + g = (result id
    r+1, gt id g+1).  radius None: the reference's ceil(0.008 * |(H, W)|) (metrics.boundary_radius).  Pixels with gt == void_label are
    removed from both maps.  native: None = the kernel for GPU tensors within its served range (radius <= 64), the torch composition
    otherwise; True = the kernel or an error; False = the composition (tools/jf_ab.py times one against the other).
    """
    if gt.dtype != torch.uint8 or res.dtype != torch.uint8:
        raise ValueError("jf_counts: label maps must be uint8")
    if gt.dim() != 3 or gt.shape != res.shape or gt.device != res.device:
        raise ValueError(f"jf_counts: expected two [T, H, W] maps of one shape and device, got {tuple(gt.shape)} and {tuple(res.shape)}")
    if radius is None:
        from ....metrics import boundary_radius
        radius = boundary_radius(gt.shape[1], gt.shape[2])
    num_gt, radius = int(num_gt), int(radius)
    if all_pairs and num_res is None:
        raise ValueError("jf_counts: all_pairs needs num_res")
    num_res = int(num_res) if all_pairs else num_gt
    if not (1 <= num_gt <= MAX_IDS and 1 <= num_res <= MAX_IDS):
        raise ValueError(f"jf_counts: between 1 and {MAX_IDS} objects and proposals")
    if radius < 1:
        raise ValueError("jf_counts: radius must be at least 1")
    if void_label is not None and not 0 <= int(void_label) <= 255:
        raise ValueError("jf_counts: void_label must fit a byte")
    if min(gt.shape) < 1:
        raise ValueError("jf_counts: empty label maps")
    if native is None:
        native = gt.is_cuda and radius <= MAX_KERNEL_RADIUS
    if not native:
        return _composition(gt, res, num_gt, num_res, radius, void_label, all_pairs)
    if not gt.is_cuda:
        raise RuntimeError("jf_counts: the kernel needs GPU tensors")
    gt, res = gt.contiguous(), res.contiguous()
    t, h, w = gt.shape
    out = torch.empty(((num_res * num_gt if all_pairs else num_gt), t, 6), dtype=torch.int32, device=gt.device)
    with torch.cuda.device(gt.device):
        check(lib().ocpg_jf_counts_u8(gt.data_ptr(), res.data_ptr(), t, h, w, num_gt, num_res, radius,
                                      -1 if void_label is None else int(void_label), int(bool(all_pairs)), out.data_ptr(), stream_ptr()),
              "ocpg_jf_counts_u8")
    return out
