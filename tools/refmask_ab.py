"""A/B of the A2D / JHMDB counts kernel (csrc/refmask_counts.hip, ocpg_refmask_counts_f32, through its binding) against the tail of
the evaluation loop it stands in for, on one GPU, in one process, the sides alternated call by call, each call between its own pair
of device events (a call's host work -- packing, the run-length loop, readbacks -- lies between them as well).

Shape: one batch of an A2D-Sentences evaluation at the 320-pixel short side: B = 2, Q = 5, frames of 320 x 428 and 320 x 568 padded to
320 x 576, original sizes equal to the augmented ones.  `up 1` feeds `pred_masks` as forward returns them ([2, 5, 320, 576]); `up 4`
feeds the stride-4 map they are the nearest x4 of ([2, 5, 80, 144], `pred_masks_low`-style), which the chain cannot use (it gets the
x4 map, made outside the timed region).

Sides:
  kernel      refmask_counts(native=True): all Q queries' (|P & G|, |P|, |G|), from which every metric follows
  entry_alone the C entry by itself (fill + kernel), ground truth and tables packed and uploaded beforehand: what of `kernel` is
              not the binding's packing
  chain       (a) A2DSentencesPostProcess's chain without the run-length strings, select_best_query, mask_iou: what P@K / IoU need
  chain_rle   (b) the same with the post-processor as it is (Q planes to the host, run-length encoded in a Python loop):
              today's engine.evaluate_referred_masks tail
The kernel is timed twice per round (`kernel`, `kernel_again`): the difference of those two medians is the spread of identical runs
that any ratio has to beat.  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F

import mask_tail_ref
from ocpg_amd import metrics
from ocpg_amd._lib import lib, stream_ptr
from ocpg_amd.models.ops.functions.refmask_func import pack_gt, refmask_counts
from ocpg_amd.models.postprocessors import A2DSentencesPostProcess

B, Q = 2, 5
PADDED = (320, 576)
SIZES = [(320, 428), (320, 568)]


def timed(fns, iters):
    """Alternate the callables; -> per-callable list of per-call milliseconds."""
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refmask_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refmask_ab.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lines = []
    post = A2DSentencesPostProcess()
    orig, size = torch.tensor(SIZES, device=dev), torch.tensor(SIZES, device=dev)
    gts = []
    for i, (h, w) in enumerate(SIZES):
        g = torch.zeros(h, w, dtype=torch.bool, device=dev)
        g[h // 4:h // 4 * 3, w // 5 + 7 * i:w // 5 * 3 + 7 * i] = True
        gts.append(g)
    scores = torch.randn(B, 1, Q, 1, generator=torch.Generator().manual_seed(0)).to(dev)

    for up in (1, 4):
        low = mask_tail_ref.logits((B * Q, PADDED[0] // up, PADDED[1] // up), "smooth", 7).view(B, Q, PADDED[0] // up, PADDED[1] // up).to(dev)
        full = F.interpolate(low, scale_factor=up) if up != 1 else low
        outputs = {"pred_logits": scores, "pred_masks": full[:, None]}

        def kern():
            return refmask_counts(low, up, SIZES, SIZES, gts, native=True)

        gt_packed, off_host = pack_gt(gts, dev)
        geom_host = torch.tensor([list(s) + list(s) for s in SIZES], dtype=torch.int32)
        geom_dev, off_dev = geom_host.to(dev), off_host.to(dev)
        raw = torch.empty((B, Q, 3), dtype=torch.int32, device=dev)

        def entry():                                                       # the C entry alone: tables and ground truth packed beforehand
            return lib().ocpg_refmask_counts_f32(low.data_ptr(), B, Q, low.shape[2], low.shape[3], up, geom_host.data_ptr(), geom_dev.data_ptr(),
                                                 gt_packed.data_ptr(), off_dev.data_ptr(), PADDED[0], PADDED[1], 0.5, 1, raw.data_ptr(), stream_ptr())

        def best_iou(preds):
            state = None
            for p, g in zip(preds, gts):
                best = metrics.select_best_query(p["scores"][None], p["masks"][None, :, 0])
                state = metrics.accumulate(state, best, g[None])
            return state

        def chain():                                                       # the post-processor's statements without rle_encode
            s = outputs["pred_logits"][:, 0, :, 0].sigmoid()
            preds = []
            for sc, m, (mh, mw), o in zip(s, outputs["pred_masks"][:, 0], SIZES, SIZES):
                m = F.interpolate(m[:, :mh, :mw].unsqueeze(1).float(), size=o, mode="bilinear", align_corners=False)
                preds.append({"scores": sc, "masks": ~(m.sigmoid() > 0.5)})
            return best_iou(preds)

        def chain_rle():
            return best_iou(post(outputs, orig, size))

        counts = kern()
        composed = refmask_counts(low, up, SIZES, SIZES, gts, native=False)
        differ = int((counts - composed).abs().max())
        assert entry() == 0 and torch.equal(raw.long(), counts)
        for _ in range(3):
            kern(), chain(), chain_rle(), entry()
        mk, ma, mb, mk2, me = timed([kern, chain, chain_rle, kern, entry], args.iters)
        sk, sa, sb, sk2, se = stats(mk), stats(ma), stats(mb), stats(mk2), stats(me)
        spread = abs(sk["median_ms"] - sk2["median_ms"]) / min(sk["median_ms"], sk2["median_ms"])
        d = {"batch": B, "queries": Q, "up": up, "source": list(low.shape[-2:]), "sizes": SIZES, "kernel": sk, "kernel_again": sk2,
             "entry_alone": se, "chain": sa, "chain_rle": sb, "identical_runs_spread": round(spread, 4),
             "kernel_over_chain": round(sk["median_ms"] / sa["median_ms"], 3), "kernel_over_chain_rle": round(sk["median_ms"] / sb["median_ms"], 3),
             "largest_count_difference_to_aten_pixels": differ,
             "device": torch.cuda.get_device_name(0)}
        print(json.dumps(d), flush=True)
        lines.append(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
