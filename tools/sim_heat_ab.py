"""A/B of the similarity-head kernel (csrc/sim_heat.hip, ocpg_sim_heat_f32) against the torch composition it stands in for
(models/ops/functions/sim_heat_func.py: normalise, one matrix product per frame, rescale, projections, scores), on one GPU, in one
process, the sides alternated call by call, each call between its own pair of device events.

Shapes: a 23 x 40 x 2048 map (720p frame, stride 32) and a 45 x 80 x 2048 map (dilated), one frame, 3 objects of 256 box candidates
each (a 16 x 16 block of cells per object), seeded positive features.  The kernel is timed twice per round (`kernel`,
`kernel_again`): the difference of those two medians is the spread of identical runs that the ratio has to beat.  Both sides go
through the public wrapper, so both pay its host work (argument checks, list uploads).  The two sides' choices are compared and the
largest plane difference is reported.

--share: one label_frames call (ResNet-101 body with random weights, one 736 x 1280 frame, 3 objects, both modes) with the head
timed inside it: the head's share of the whole, so nobody reads the per-kernel ratio as an end-to-end one.

One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from ocpg_amd.models.ops.functions import sim_heat_func
from ocpg_amd.models.ops.functions.sim_heat_func import sim_heat

SHAPES = {"23x40x2048": (23, 40, 2048), "45x80x2048": (45, 80, 2048)}
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


def inputs(h, w, c, dev):
    g = np.random.default_rng(0)
    feat = torch.from_numpy((np.abs(g.standard_normal((1, h, w, c))) + 0.05).astype(np.float32)).to(dev)
    xy, boxes = [], []
    for o in range(OBJECTS):
        x0, y0 = 2 + 7 * o, 1 + 2 * o
        xy += [(x, y) for x in range(x0, x0 + 16) for y in range(y0, y0 + 16)]
        boxes.append([x0, y0, x0 + 16, y0 + 16])
    return (feat, torch.zeros(OBJECTS, dtype=torch.int32), torch.arange(OBJECTS + 1, dtype=torch.int32) * 256,
            torch.tensor(xy, dtype=torch.int32), torch.tensor(boxes, dtype=torch.int32))


def head_share(dev, emit, iters):
    from ocpg_amd.weak_labels import SimilarityLabeler
    torch.manual_seed(0)
    fh, fw = 736, 1280
    frames = torch.randn(1, 3, fh, fw, device=dev)
    centers = torch.tensor([[[300, 200], [700, 400], [1000, 600]]])
    boxes = torch.tensor([[[100, 60, 620, 420], [500, 200, 1000, 700], [900, 500, 1270, 730]]])
    valid = torch.ones(1, 3, dtype=torch.int64)
    for native in (False, True):
        lab = SimilarityLabeler("resnet101", frames_per_pass=1, native=native).to(dev)
        head_ms = []
        inner = sim_heat_func.sim_heat

        def spy(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = inner(*a, **k)
            e1.record()
            head_ms.append((e0, e1))
            return r

        import ocpg_amd.weak_labels as wl
        wl.sim_heat = spy
        try:
            for _ in range(2):
                lab.label_frames(frames, centers, boxes, valid)
            whole, head = [], []
            for _ in range(iters):
                head_ms.clear()
                (ms,) = timed([lambda: lab.label_frames(frames, centers, boxes, valid)], 1)
                whole.append(ms[0])
                head.append(sum(a.elapsed_time(b) for a, b in head_ms))
        finally:
            wl.sim_heat = inner
        emit({"measurement": "label_frames", "backbone": "resnet101 fp32, random weights", "frame": [fh, fw], "objects": 3,
              "head": "kernel" if native else "composition", "whole_call": stats(whole), "head_both_modes": stats(head),
              "head_share_of_call": round(statistics.median(head) / statistics.median(whole), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="23x40x2048,45x80x2048")
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_heat_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_heat_ab.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for shape in [s for s in args.shapes.split(",") if s]:
        h, w, c = SHAPES[shape]
        feat, obj_frame, off, xy, box = inputs(h, w, c, dev)

        def comp():
            return sim_heat(feat, obj_frame, off, xy, box, native=False)

        def kern():
            return sim_heat(feat, obj_frame, off, xy, box, native=True)

        a, b = comp(), kern()
        same = bool(torch.equal(a[1], b[1]))
        diff = float((a[0] - b[0]).abs().max()) if same else None
        for _ in range(2):
            comp(), kern()
        mc, mk, mk2 = timed([comp, kern, kern], args.iters)
        sc, sk, sk2 = stats(mc), stats(mk), stats(mk2)
        spread = abs(sk["median_ms"] - sk2["median_ms"]) / min(sk["median_ms"], sk2["median_ms"])
        emit({"measurement": "head", "shape": shape, "frames": 1, "objects": OBJECTS, "candidates_per_object": 256, "mode": "box",
              "composition": sc, "kernel": sk, "kernel_again": sk2, "speedup_median": round(sc["median_ms"] / sk["median_ms"], 2),
              "identical_runs_spread": round(spread, 4), "choices_equal": same, "max_plane_difference": diff})
    if args.share:
        head_share(dev, emit, max(3, args.iters // 4))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
