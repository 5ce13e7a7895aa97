"""Seeded inputs the CPU and GPU tests of refmask_counts share (csrc/refmask_counts.hip), and their float64 expectations built on
tests/mask_tail_ref.py: per plane the referee's decision wherever it can decide, so a count of P is bounded by

    sum(want & decided [& G])  <=  count  <=  that + sum(~decided [& G])

A case is one batch.  Its sizes are given on the VIRTUAL map (vh x vw, multiples of 4): at up 4 the source is [B, Q, vh / 4, vw / 4],
at up 1 it is [B, Q, vh, vw]; crops and original sizes are the same for both.
"""
import functools

import torch

import mask_tail_ref as R

# name -> (virtual size, Q, kind, [(crop, original size)], seed)
CASES = {
    # three samples, different crops and original sizes, none a multiple of 4; the middle one's ground truth is empty
    "three-sizes": ((24, 36), 5, "smooth", [((22, 33), (45, 70)), ((18, 26), (37, 53)), ((23, 35), (30, 41))], 3),
    # the second sample's out_h and out_w lie well below the batch maximum
    "small-in-big": ((24, 36), 5, "smooth", [((22, 33), (90, 131)), ((10, 14), (9, 13))], 5),
    # more than one workgroup along x; Q = 1
    "wide": ((4, 300), 1, "smooth", [((3, 298), (3, 1030))], 4),
    "rough": ((80, 100), 2, "rough", [((80, 100), (160, 200)), ((77, 93), (101, 67))], 2),
    # plane (0, 2) is negative everywhere: |P| = 0 without invert, out_h * out_w with it
    "saturated": ((24, 36), 5, "saturated", [((22, 33), (45, 70)), ((24, 36), (24, 36))], 1),
}
EMPTY_GT = {"three-sizes": 1}
ALL_NEGATIVE = {"saturated": (0, 2)}
UPS = (4, 1)
THR = 0.5


def source(name, up):
    (vh, vw), q, kind, samples, seed = CASES[name]
    b = len(samples)
    if kind == "saturated":
        # signs drawn per stride-4 cell and replicated: at up 1 a sign per pixel would put a +-100 transition, and with it undecidable
        # pixels, between every two pixels
        src = R.logits((b * q, vh // 4, vw // 4), kind, 1000 * seed).view(b, q, vh // 4, vw // 4)
        src = src.repeat_interleave(4 // up, 2).repeat_interleave(4 // up, 3).contiguous()
    else:
        src = R.logits((b * q, vh // up, vw // up), kind, 1000 * seed + up).view(b, q, vh // up, vw // up)
    if name in ALL_NEGATIVE:
        i, j = ALL_NEGATIVE[name]
        src[i, j] = -src[i, j].abs() - 1.0
    return src


def ground_truth(name):
    """One bool mask per sample: a coarse uniform field, nearest-upsampled by 8 and thresholded -- blobs with straight edges."""
    _, _, _, samples, seed = CASES[name]
    g = torch.Generator().manual_seed(77 + seed)
    out = []
    for i, (_, (h, w)) in enumerate(samples):
        coarse = torch.rand((h + 7) // 8 + 1, (w + 7) // 8 + 1, generator=g) > 0.5
        m = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1)[3:3 + h, 5:5 + w].clone()
        if EMPTY_GT.get(name) == i:
            m.zero_()
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def expectation(name, up):
    """-> list over samples of (want bool [Q, H0, W0] at THR without invert, decided bool [Q, H0, W0]); computed once per process."""
    src = source(name, up)
    out = []
    for b, (crop, size) in enumerate(CASES[name][3]):
        want, decided = R.binary_decision(R.referee(src[b], up, crop, size), THR)
        out.append((want, decided))
    return out


def bounds(name, up, invert):
    """-> (lo, hi) int64 [B, Q, 3]: the range each count may take (equal for |G|, and wherever the referee decides every pixel)."""
    gts = ground_truth(name)
    lo, hi = [], []
    for (want, decided), g in zip(expectation(name, up), gts):
        want = ~want if invert else want
        sure, open_ = want & decided, ~decided
        n_g = g.sum().expand(want.shape[0])
        l = torch.stack([(sure & g).flatten(1).sum(1), sure.flatten(1).sum(1), n_g], 1)
        h = l + torch.stack([(open_ & g).flatten(1).sum(1), open_.flatten(1).sum(1), torch.zeros_like(n_g)], 1)
        lo.append(l)
        hi.append(h)
    return torch.stack(lo), torch.stack(hi)
