"""Float64 referee of the mask tail (csrc/mask_tail.hip, include/ocpg_hip.h: ocpg_mask_tail_f32) with its error bound, and the
seeded inputs the CPU and GPU tests share.

The referee restates the contract in float64 with EXACT coordinates: virtual map V[y][x] = src[y // up][x // up] cropped to
crop_h x crop_w, bilinear sample under the align_corners=False rule, sigmoid.  An fp32 evaluation differs from it by

    B = 4 eps32 (s_y + 1) G_y + 4 eps32 (s_x + 1) G_x + 8 eps32 M            on the logit
    0.25 B + 4 eps32                                                         on the probability

s = source coordinate of the pixel, G = largest neighbour difference of the plane's virtual map in that direction, M = max |V| of the
plane.  First two terms: the fp32 coordinate scale * (d + 0.5) - 0.5 carries at most ~3 roundings of relative size eps32 on values
<= s + 1 (4 eps32 (s + 1) with margin), and bilinear interpolation is continuous and piecewise linear in the coordinate with slope
<= G, so a coordinate error -- including one that flips the floor -- moves the value by at most error x G.  Third term: the weights
l0 = 1 - l1 and the 6 multiplies / 3 adds of the blend, each a relative eps32 / 2 on terms bounded by M.  0.25 is the sigmoid's
largest slope; 4 eps32 covers expf (a few ulp), the add and the division on a result <= 1.
"""
import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23

# (source shape [N, hs, ws], up, crop, out, kind of logits)
CASES = [
    ((2, 5, 7), 4, (18, 26), (37, 53), "smooth"),        # upscale, nothing a multiple of 4
    ((2, 5, 7), 4, (18, 26), (9, 13), "smooth"),         # downscale
    ((2, 5, 7), 1, (5, 7), (5, 7), "smooth"),            # identity: sigmoid(src)
    ((1, 2, 3), 4, (1, 1), (3, 4), "smooth"),            # every clamp
    ((1, 2, 300), 1, (2, 300), (2, 1030), "smooth"),     # more than one workgroup along x
    ((3, 20, 26), 4, (80, 100), (160, 200), "rough"),    # randn * 8, N = 3
    ((2, 6, 9), 4, (22, 33), (45, 70), "saturated"),     # logits +-100
]


def case_id(case):
    shape, up, crop, out, kind = case
    return "{}-up{}-{}x{}-to-{}x{}-{}".format("x".join(map(str, shape)), up, crop[0], crop[1], out[0], out[1], kind)


def logits(shape, kind, seed):
    """fp32 source logits [N, hs, ws].  smooth: bicubic blow-up of a coarse normal field x 6 + 0.5 randn; rough: randn x 8;
    saturated: +-100 with the sign of a normal field."""
    g = torch.Generator().manual_seed(seed)
    n, hs, ws = shape
    if kind == "rough":
        return torch.randn(n, hs, ws, generator=g) * 8
    if kind == "saturated":
        return torch.sign(torch.randn(n, hs, ws, generator=g)) * 100
    coarse = torch.randn(n, 1, max(2, math.ceil(hs / 4)), max(2, math.ceil(ws / 4)), generator=g)
    field = F.interpolate(coarse, size=(hs, ws), mode="bicubic", align_corners=False)[:, 0]
    return field * 6 + 0.5 * torch.randn(n, hs, ws, generator=g)


def _axis(crop, out):
    s = (torch.arange(out, dtype=torch.float64) + 0.5) * (crop / out) - 0.5
    s = s.clamp(min=0)
    i0 = s.floor().long().clamp(max=crop - 1)
    i1 = i0 + (i0 < crop - 1).long()
    l1 = s - i0
    return s, i0, i1, l1


def referee(src, up, crop, out_size):
    """src [..., hs, ws] (any float dtype; read exactly) -> dict of float64 tensors [..., out_h, out_w]:
    v (logit), p (probability), bound_v (B above), bound_p."""
    v64 = src.double().repeat_interleave(up, -2).repeat_interleave(up, -1)[..., :crop[0], :crop[1]]
    sy, y0, y1, ly = _axis(crop[0], out_size[0])
    sx, x0, x1, lx = _axis(crop[1], out_size[1])
    r0, r1 = v64.index_select(-2, y0), v64.index_select(-2, y1)
    a, b = r0.index_select(-1, x0), r0.index_select(-1, x1)
    c, d = r1.index_select(-1, x0), r1.index_select(-1, x1)
    ly, lx = ly[:, None], lx[None, :]
    v = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)
    lead = v64.shape[:-2]
    zero = torch.zeros(lead, dtype=torch.float64)
    gy = (v64[..., 1:, :] - v64[..., :-1, :]).abs().flatten(-2).max(-1)[0] if crop[0] > 1 else zero
    gx = (v64[..., :, 1:] - v64[..., :, :-1]).abs().flatten(-2).max(-1)[0] if crop[1] > 1 else zero
    m = v64.abs().flatten(-2).max(-1)[0]
    bound_v = (4 * EPS32 * (sy[:, None] + 1) * gy[..., None, None] + 4 * EPS32 * (sx[None, :] + 1) * gx[..., None, None]
               + 8 * EPS32 * m[..., None, None])
    return {"v": v, "p": torch.sigmoid(v), "bound_v": bound_v, "bound_p": 0.25 * bound_v + 4 * EPS32}


def binary_decision(ref, thr):
    """-> (decision bool [...], decided bool [...]): p > thr where the fp64 probability is further than its bound from the
    threshold (thr as the fp32 value the entry point receives)."""
    thr = float(torch.tensor(thr, dtype=torch.float32))
    return ref["p"] > thr, (ref["p"] - thr).abs() > ref["bound_p"]


def label_decision(ref, thr, bg):
    """ref of a [K, N, hs, ws] source -> (labels uint8 [N, h, w], decided bool [N, h, w]) under inference_davis.py:253-261's rule
    (first maximum of [bg, p_1 .. p_K] with p_k < thr zeroed).  A pixel is decided when every p_k is further than its bound from the
    threshold and the winner leads the runner-up by more than the two candidates' bounds together (bg and a zeroed candidate are
    exact).  Candidates with bit-identical values everywhere (a deliberate tie) are not each other's runner-up: the first wins."""
    thr = float(torch.tensor(thr, dtype=torch.float32))
    bg = float(torch.tensor(bg, dtype=torch.float32))
    p, bp = ref["p"], ref["bound_p"]
    keep = p >= thr
    cand = torch.cat([torch.full_like(p[:1], bg), torch.where(keep, p, torch.zeros_like(p))], 0)
    cb = torch.cat([torch.zeros_like(bp[:1]), torch.where(keep, bp, torch.zeros_like(bp))], 0)
    labels = cand.argmax(0)
    decided = ((p - thr).abs() > bp).all(0)
    top = cand.gather(0, labels[None])[0]
    topb = cb.gather(0, labels[None])[0]
    for k in range(cand.shape[0]):
        other = labels != k
        same = (cand[k] == top) & (k > labels)                     # an exact duplicate behind the winner loses by the tie rule
        lead = (top - cand[k]) > (topb + cb[k])
        decided &= ~other | lead | same
    return labels.to(torch.uint8), decided


# ---- inputs of the decision tests (modes 1 / 2) ---------------------------------------------------------------------------------
BINARY_CASES = [CASES[0], CASES[4], CASES[5]]
# (K, source shape [N, hs, ws], up, crop, out, seed).  Where two objects both saturate (logits beyond ~15) their probabilities sit
# within 4 eps32 of each other and the winner is undecidable by construction; the seeds are ones whose fields leave at most 0.5 %
# of the pixels in that state and give every label a region (both are properties of the inputs, asserted by the CPU test).
LABEL_CASES = [
    (1, (2, 9, 13), 4, (34, 50), (67, 101), 2),
    (3, (2, 9, 13), 4, (34, 50), (67, 101), 10),
    (3, (1, 3, 70), 4, (10, 270), (13, 301), 16),         # more than one workgroup along x
]


def label_sources(k, shape, seed):
    """[K, N, hs, ws] smooth logits, one independent field per object."""
    return torch.stack([logits(shape, "smooth", seed * 100 + i) for i in range(k)])
