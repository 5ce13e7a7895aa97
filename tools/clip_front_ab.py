"""A/B of the Pillow-exact clip front end (csrc/clip_front.hip, pil_exact=True) against the float pipelines it is an alternative to, on
one GPU, in one process, the two sides alternated call by call, each call between its own pair of device events.

(a) eval:  eval_pipeline() against eval_pipeline(pil_exact=True) on uint8 clips of 36 x 480 x 854 and 36 x 720 x 1280, both to 360 x 640.
(b) train: the cropped branch of train_pipeline() against train_pipeline(pil_exact=True) on a uint8 clip of 5 x 480 x 854, both sides
           with the same seeds (seeds whose first draw selects the cropped branch), with a minimal target (boxes and a caption), so the
           time is the frames'.  Two sweeps over the same seeds: in the first every call meets a crop geometry for the first time, so
           the exact side also builds and uploads its coefficient tables (host work inside the timed interval); in the second they
           are resident.

One JSON line per measurement: median / min of the per-call times, the ocpg_clip_front_u8 launches of one exact call (call census), the
kernel's modelled bytes (every window byte read once, every output element written once; tables and the tiles' shared tap rows are
not counted) and how far the two sides' pixels are apart.  A time is a device-event interval around everything a call enqueues, so
the float path's launches and their gaps count, as they do for a user.  The two sides do NOT compute the same thing: the exact side
returns Pillow's bytes, the float side the unrounded filter.
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from ocpg_amd import _lib
from ocpg_amd.datasets.clip_transforms import IMAGENET_MEAN, IMAGENET_STD, eval_pipeline, train_pipeline


def timed(fns, iters):
    """Alternate the callables; -> per-callable list of per-call milliseconds."""
    ms = [[] for _ in fns]
    for it in range(iters):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(it)
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "calls": len(ms)}


def launches(fn):
    calls = _lib.census(True)
    fn(0)
    _lib.census(False)
    return dict(calls)


def grey_levels(x):
    """normalised fp32 [T, 3, h, w] -> the 0..255 scale"""
    m = torch.tensor(IMAGENET_MEAN, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(IMAGENET_STD, device=x.device).view(1, 3, 1, 1)
    return (x * s + m) * 255.0


def difference(a, b):
    ga, gb = grey_levels(a), grey_levels(b)
    return {"max_abs_diff_grey_levels": round((ga - gb).abs().max().item(), 4),
            "pixels_differing_after_rounding": round((ga.round() != gb.round()).float().mean().item(), 4)}


def eval_ab(dev, iters, emit):
    for t, h, w in ((36, 480, 854), (36, 720, 1280)):
        clip = torch.randint(0, 256, (t, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
        old, new = eval_pipeline(), eval_pipeline(pil_exact=True)
        fns = [lambda it: old(clip, None), lambda it: new(clip, None)]
        a, b = fns[0](0)[0], fns[1](0)[0]
        oh, ow = b.shape[-2:]
        diff = difference(a, b)
        del a, b
        for _ in range(3):
            fns[0](0), fns[1](0)
        mo, mn = timed(fns, iters)
        so, sn = stats(mo), stats(mn)
        model = t * 3 * (h * w + 4 * oh * ow)
        emit({"part": "eval", "frames": t, "in": [h, w], "out": [oh, ow], "float_pipeline": so, "pil_exact": sn,
              "ratio_float_over_exact_median": round(so["median_ms"] / sn["median_ms"], 3), "pil_exact_launches": launches(fns[1]),
              "model_bytes_clip_front": model, "clip_front_model_gbs": round(model / sn["median_ms"] / 1e6, 1), **diff})


def train_ab(dev, iters, emit):
    t, h, w = 5, 480, 854
    clip = torch.randint(0, 256, (t, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    target = {"boxes": torch.tensor([[100.0, 80.0, 500.0, 400.0]]).repeat(t, 1), "caption": "the dog on the left", "size": torch.tensor([h, w])}
    seeds = [s for s in range(1000) if not random.Random(s).random() < 0.5][:iters + 3]          # first draw: the cropped branch
    old, new = train_pipeline(), train_pipeline(pil_exact=True)
    fns = [lambda it: old(clip, dict(target), random.Random(seeds[it])), lambda it: new(clip, dict(target), random.Random(seeds[it]))]
    for i in range(3):
        fns[0](iters + i), fns[1](iters + i)
    a, b = None, None
    for tables in ("first use of every crop geometry", "resident"):            # the second sweep repeats the first one's seeds
        mo, mn = timed(fns, iters)
        so, sn = stats(mo), stats(mn)
        if a is None:
            a, b = fns[0](0)[0], fns[1](0)[0]
        emit({"part": "train_cropped_branch", "frames": t, "in": [h, w], "seeds": iters, "resample_tables": tables, "float_pipeline": so,
              "pil_exact": sn, "ratio_float_over_exact_median": round(so["median_ms"] / sn["median_ms"], 3),
              "pil_exact_launches": launches(fns[1]), "same_output_size": list(a.shape) == list(b.shape), **difference(a, b)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_front_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parts", default="eval,train")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_front_ab: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        parts = a.parts.split(",")
        if "eval" in parts:
            eval_ab(dev, a.iters, emit)
        if "train" in parts:
            train_ab(dev, a.iters, emit)


if __name__ == "__main__":
    main()
