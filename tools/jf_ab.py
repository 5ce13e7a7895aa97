"""A/B of the J&F counts kernel (csrc/jf_metrics.hip, ocpg_jf_counts_u8) against the torch composition it stands in for
(models/ops/functions/jf_func.py: shifts for the boundary map, conv2d with the disk for the dilation), on one GPU, in one process,
the sides alternated call by call, each call between its own pair of device events.

Shapes: DAVIS (3 objects, 3 proposals, 70 frames of 480 x 854, radius 8) and 1080p (20 frames of 1080 x 1920, radius 18), diagonal
pairs and all pairs; smooth-noise label maps of tests/jf_ref.py (four distinct frames, shifted from frame to frame), the result the ground truth rolled by radius + 1 with a void stripe.
The kernel is timed twice per round (`kernel`, `kernel_again`): the difference of those two medians is the spread of identical runs
that the ratio has to beat.  The two sides' counts are compared exactly.  `referee_cpu` is the numpy / scipy referee (what the
reference's host evaluator does: two dilations per pair and frame) for ONE pair on ONE frame on this machine's CPU, multiplied by
pairs x frames: context, not a GPU figure.

One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import jf_ref
from ocpg_amd.metrics import boundary_radius
from ocpg_amd.models.ops.functions.jf_func import jf_counts

SHAPES = {"davis": (70, 480, 854), "1080p": (20, 1080, 1920)}
OBJECTS = 3


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="davis,1080p")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jf_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jf_ab.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for shape in args.shapes.split(","):
        T, H, W = SHAPES[shape]
        radius = boundary_radius(H, W)
        few = jf_ref.blobs(1, 4, H, W, OBJECTS, sigma=24.0)           # four distinct frames, moved about to fill the clip
        gt_h = np.stack([np.roll(few[t % 4], (3 * t, 5 * t), axis=(0, 1)) for t in range(T)])
        res_h = np.roll(gt_h, (radius + 1, -(radius + 1)), axis=(1, 2))
        gt_h[:, :, W // 3:W // 3 + 6] = 255
        gt, res = torch.from_numpy(gt_h).to(dev), torch.from_numpy(res_h).to(dev)
        t0 = time.perf_counter()
        ref = jf_ref.reference_counts(gt_h[:1], res_h[:1], 1, 1, radius, 255, False)
        ref_s = time.perf_counter() - t0
        for all_pairs in (False, True):
            def comp():
                return jf_counts(gt, res, OBJECTS, OBJECTS, radius=radius, void_label=255, all_pairs=all_pairs, native=False)

            def kern():
                return jf_counts(gt, res, OBJECTS, OBJECTS, radius=radius, void_label=255, all_pairs=all_pairs, native=True)

            a, b = comp(), kern()
            equal = bool(torch.equal(a, b))
            for _ in range(2):
                comp(), kern()
            mc, mk, mk2 = timed([comp, kern, kern], args.iters)
            sc, sk, sk2 = stats(mc), stats(mk), stats(mk2)
            spread = abs(sk["median_ms"] - sk2["median_ms"]) / min(sk["median_ms"], sk2["median_ms"])
            pairs = OBJECTS * OBJECTS if all_pairs else OBJECTS
            emit({"shape": shape, "frames": T, "size": [H, W], "radius": radius, "objects": OBJECTS, "proposals": OBJECTS,
                  "pairs": "all" if all_pairs else "diagonal", "composition": sc, "kernel": sk, "kernel_again": sk2,
                  "speedup_median": round(sc["median_ms"] / sk["median_ms"], 2), "identical_runs_spread": round(spread, 4),
                  "counts_equal": equal, "kernel_equals_referee_on_first_pair_and_frame": bool(np.array_equal(b[:1, :1].cpu().numpy(), ref)),
                  "referee_cpu": {"one_pair_one_frame_seconds": round(ref_s, 3), "times_pairs_times_frames_seconds": round(ref_s * pairs * T, 1)}})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
