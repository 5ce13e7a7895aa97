"""The target pack's torch composition (ocpg_amd/models/ops/functions/target_pack_func.py, native=False -- the reference the HIP kernel
is held to bit for bit) against an independent numpy loop implementation: literal Python slices for the box, numpy for the heat
weight, the nearest resize by its index formula."""
import numpy as np
import pytest
import torch

from ocpg_amd.models.ops.functions.target_pack_func import build_target_pack

F32 = np.float32


def ceil32(v):
    return (v + 31) // 32 * 32


def make_targets(shapes, T, boxes, heat_kind="random", labels=True, seed=0, sizes=None, zero_valid=None):
    """shapes: (H, W) per clip; boxes: [B][T] cxcywh rows; heat_kind: 'random' (values straddling 0.3 / 0.5 / 0.7, the three
    thresholds themselves included), 'const' (one value everywhere, padding included: hi == lo) or 'outside' (non-zero only
    outside the box)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (h, w) in enumerate(shapes):
        size = torch.tensor(sizes[i] if sizes else (h, w))
        bx = torch.tensor(boxes[i], dtype=torch.float32).reshape(T, 4)
        if heat_kind == "const":
            heat = torch.full((T, h, w), 0.25)       # below the clamp, like the zero padding: a = 0.2 everywhere
        else:
            heat = torch.rand((T, h, w), generator=g)
            heat[:, 0, :3] = torch.tensor([0.3, 0.5, 0.7])
            if heat_kind == "outside":
                heat[:, : h // 2] = 0.0              # the boxes of this kind lie in the upper half
        d = {"size": size, "valid": torch.ones(T, dtype=torch.long), "boxes": bx,
             "masks": (torch.rand((T, h, w), generator=g) > 0.5).float(), "weights": heat,
             "weak_masks": (torch.rand((T, h, w), generator=g) > 0.3).float()}
        if zero_valid == i:
            d["valid"] = torch.zeros(T, dtype=torch.long)
        if labels:
            d["labels"] = torch.randint(0, 5, (T,), generator=g)
        out.append(d)
    return out


# ordinary | zero width after truncation | x0 < 0 after truncation (wrap-around) | past the image edge | the full image
ORDINARY, ZERO_W, WRAP, PAST_EDGE, FULL = ([0.4, 0.45, 0.3, 0.5], [0.507, 0.5, 0.004, 0.4], [0.1, 0.5, 0.5, 0.4], [0.9, 0.8, 0.4, 0.6],
                                           [0.5, 0.5, 1.0, 1.0])
UPPER = [0.5, 0.2, 0.6, 0.3]       # lies in the upper half of the clip ('outside' heat maps)


def numpy_pack(targets, s, sl, sm, ls_hw):
    B, T = len(targets), targets[0]["masks"].shape[0]
    PH = ceil32(max(t["masks"].shape[1] for t in targets))
    PW = ceil32(max(t["masks"].shape[2] for t in targets))

    def padded(key):
        out = np.zeros((B, T, PH, PW), F32)
        for i, t in enumerate(targets):
            a = t[key].numpy().astype(F32)
            out[i, :, : a.shape[1], : a.shape[2]] = a
        return out

    gt, heat, weak = padded("masks"), padded("weights"), padded("weak_masks")
    region = np.zeros((B, T, PH, PW), F32)
    for i, t in enumerate(targets):
        h, w = (int(v) for v in t["size"])
        for f in range(T):
            cx, cy, bw, bh = (F32(v) for v in t["boxes"][f].numpy())
            x0, x1 = int(F32(cx - F32(0.5) * bw) * F32(w)), int(F32(cx + F32(0.5) * bw) * F32(w))      # int(): toward zero
            y0, y1 = int(F32(cy - F32(0.5) * bh) * F32(h)), int(F32(cy + F32(0.5) * bh) * F32(h))
            if y1 - y0 > 0 and x1 - x0 > 0:
                region[i, f][y0:y1, x0:x1] = 1

    def sub(x, k):
        return x[..., k // 2::k, k // 2::k]

    def heat_weight(hm, reg):
        a = np.abs(np.clip(hm, F32(0.3), F32(0.7)) - F32(0.5))
        lo, hi = a.min(), a.max()
        wgt = (a - lo) / F32(F32(hi - lo) + F32(1e-5))
        return np.where(reg == 0, F32(1), wgt).astype(F32)

    region_s, region_l = sub(region, s), sub(region, sl)
    ih, iw = region_s.shape[-2:]
    lh, lw = ls_hw
    ys = [min(int(np.floor(F32(y) * (F32(ih) / F32(lh)))), ih - 1) for y in range(lh)]
    xs = [min(int(np.floor(F32(x) * (F32(iw) / F32(lw)))), iw - 1) for x in range(lw)]
    region_ls = np.zeros((B * T, lh, lw), F32)
    for n in range(B * T):
        for y in range(lh):
            for x in range(lw):
                region_ls[n, y, x] = region_s[n // T, n % T, ys[y], xs[x]]
    return dict(gt_s=sub(gt, s), gt_m=sub(gt, sm), region_s=region_s, region_l=region_l, region_ls=region_ls,
                weak_s=sub(weak, s) * region_s, weak_l=sub(weak, sl) * region_l, w_s=heat_weight(sub(heat, s), region_s),
                w_l=heat_weight(sub(heat, sl), region_l), tboxes=np.stack([t["boxes"].numpy() for t in targets]),
                valid_f=np.stack([t["valid"].numpy() for t in targets]).astype(F32),
                valid_i=np.stack([t["valid"].numpy() for t in targets]),
                labels=np.stack([t["labels"].numpy() for t in targets]) if "labels" in targets[0] else None)


def check(targets, s, sl, sm, ls_hw):
    p = build_target_pack(targets, s, sl, sm, ls_hw, native=False)
    ref = numpy_pack(targets, s, sl, sm, ls_hw)
    assert p.targets is targets and p.key == (s, sl, sm, tuple(ls_hw))
    for k, r in ref.items():
        got = getattr(p, k)
        if r is None:
            assert got is None, k
            continue
        assert tuple(got.shape) == r.shape, (k, tuple(got.shape), r.shape)
        assert np.array_equal(got.numpy(), r), k


@pytest.mark.parametrize("strides", [(1, 2, 2), (2, 4, 2)])
@pytest.mark.parametrize("ls_hw", [(16, 24), (20, 28)])
def test_ragged_clips_against_numpy_loops(strides, ls_hw):
    t = make_targets([(40, 72), (33, 96)], 2, [[ORDINARY, ZERO_W], [WRAP, PAST_EDGE]], zero_valid=1)
    check(t, *strides, ls_hw)


@pytest.mark.parametrize("heat_kind,labels", [("const", False), ("outside", True)])
def test_single_clip_heat_maps(heat_kind, labels):
    t = make_targets([(32, 32)], 1, [[FULL if heat_kind == "const" else UPPER]], heat_kind=heat_kind, labels=labels)
    check(t, 1, 2, 2, (16, 24))
    if heat_kind == "const":       # hi == lo: the divisor is the 1e-5 alone and the weights are 0 (inside the full-image box)
        assert float(build_target_pack(t, 1, 2, 2, (16, 24), native=False).w_s.max()) == 0.0


def test_box_scaled_by_a_size_beyond_the_map():
    t = make_targets([(40, 72)], 2, [[PAST_EDGE, WRAP]], sizes=[(80, 120)])
    check(t, 1, 2, 2, (20, 28))
