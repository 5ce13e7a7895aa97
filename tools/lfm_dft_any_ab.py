"""A/B of the LFM block's own transforms on the map sizes csrc/lfm_dft.hip refuses (csrc/lfm_dft_any.hip, OCPG_LFM_DFT_ANY=1) against the
route the parent took for them (rocFFT between the transposing kernels, OCPG_LFM_DFT_ANY=0), on one GPU, in one process, the two sides
alternated call by call, each call between its own pair of device events, operands cold (a buffer larger than L2 + MALL is rewritten
before every timed call, outside the events).

(a) block:   one LFMResizeAdaptive(256, 7), forward + backward, bf16 autocast as in training, at the shapes the recipes produce.  The input
             is in the memory GroupNorm hands over at such a size (planes, NCHW: groupnorm_func keeps channels-last for the old predicate
             only), so the own route pays one channels-last copy; "own_nhwc_input" is the same route fed channels-last memory (what is left
             once that copy is gone) and "nhwc_copy" the copy alone.  24 x 40 is an old-served neighbour (both settings run lfm_dft.hip).
(a') sweep:  the same A/B at N = 10 on 40 x p and p x 40 for every prime 17 <= p <= 127: where the O(p^2) direct stage stops paying
             (modules.DFT_ANY_MAX_PRIME and dft_any_default follow from these lines), and a few lengths above 128 (32 channels per workgroup).
(b) forward: one eval forward of the config-#2 model (ResNet-101, 4 + 4 layers, 5 queries, bf16 autocast, initial weights) on 36 frames
             of 360 x 640, both settings alternated; the outputs are compared.

One JSON line per measurement: median / min of the per-call times and their spread, per-entry-point counts, what the outputs differ by.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from ocpg_amd import _lib
from ocpg_amd.models import fallbacks, modules
from ocpg_amd.models.ops.functions import spectral_func as sf

C = 256
TRAIN = [(10, 23, 40), (10, 40, 71), (10, 44, 79), (10, 46, 80)]
EVAL = [(36, 23, 40), (36, 46, 80), (36, 60, 107)]
NEIGHBOUR = [(10, 24, 40)]
LONG = [(10, 40, 130), (10, 40, 134), (10, 40, 146), (10, 40, 160), (10, 40, 250), (10, 40, 256), (10, 136, 40), (10, 146, 40), (10, 256, 40)]   # 32-channel slabs
SWEEP = [17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127]     # every prime a direct stage of <= 128 can have


def timed(fns, iters, before=None):
    """Alternate the callables; -> per-callable list of per-call milliseconds."""
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "calls": len(ms)}


def block_ab(dev, iters, emit, groups):
    torch.manual_seed(0)
    lfm = modules.LFMResizeAdaptive(C, 7).to(dev)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)       # 1 GiB: past the 256 MB MALL

    def cold():
        flush.add_(1)

    default, modules.dft_any_default = modules.dft_any_default, lambda n: True        # every length the kernels serve is measured: the default follows
    for kind, shapes in groups:
        for n, h, w in shapes:
            planes = torch.randn(n, C, h, w, device=dev)
            nhwc = planes.contiguous(memory_format=torch.channels_last)
            go = torch.randn(n, C, h, w, device=dev)

            def run(on, src, keep=False):
                modules.DFT_ANY = on
                x = src.detach().requires_grad_(True)
                lfm.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y, _ = lfm(x)
                y.backward(go)
                return (y.detach(), x.grad) if keep else None

            calls = _lib.census(True)
            own = run(True, planes, True)
            _lib.census(False)
            counts = {k: v for k, v in calls.items() if k.startswith("ocpg_lfm_spectrum")}
            libr = run(False, planes, True)
            diff = {"out_max_abs_diff": (own[0] - libr[0]).abs().max().item(), "out_max_abs": libr[0].abs().max().item(),
                    "gx_max_abs_diff": (own[1] - libr[1]).abs().max().item(), "gx_max_abs": libr[1].abs().max().item()}
            del own, libr
            fns = [lambda: run(True, planes), lambda: run(False, planes), lambda: run(True, nhwc), lambda: run(False, planes),
                   lambda: sf._nhwc32(planes)]
            for fn in fns:
                for _ in range(3):
                    fn()
            res = [stats(m) for m in timed(fns, iters, cold)]
            emit({"part": "block", "kind": kind, "N": n, "C": C, "h": h,"w": w, "plan_h": sf._axis_plan(h), "plan_w": sf._axis_plan(w),
                  "own_served_by_old_kernels": sf.dft_supported(h, w), "own": res[0], "library": res[1], "own_nhwc_input": res[2],
                  "library_again": res[3], "nhwc_copy": res[4], "library_over_own_median": round(res[1]["median_ms"] / res[0]["median_ms"], 3),
                  "identical_runs_spread": round(abs(res[1]["median_ms"] - res[3]["median_ms"]) / res[1]["median_ms"], 4), "entry_points_own": counts, **diff})
    modules.DFT_ANY, modules.dft_any_default = True, default


def forward_ab(dev, iters, emit):
    from ocpg_amd.models import build_model
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    T, H, W = 36, 360, 640
    torch.manual_seed(0)
    args = bench.model_args(dev, "resnet101", amp=True)
    args.dataset_file = "davis"
    model, _, _ = build_model(args)
    model.to(dev).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    frames = torch.randn(T, 3, H, W, device=dev)
    text = PrecomputedText(torch.randn(1, 9, 768, device=dev), torch.randn(1, 768, device=dev), torch.zeros(1, 9, dtype=torch.bool, device=dev))
    targets = [{"size": torch.as_tensor([H, W], device=dev)}]

    def run(on):
        modules.DFT_ANY = on
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model([frames], text, targets)

    fallbacks.reset()
    calls = _lib.census(True)
    a = run(True)
    _lib.census(False)
    counts = {k: v for k, v in calls.items() if k.startswith("ocpg_lfm_spectrum")}
    b = run(False)
    diff = {"pred_masks_max_abs_diff": (a["pred_masks"].float() - b["pred_masks"].float()).abs().max().item(),
            "pred_masks_max_abs": b["pred_masks"].float().abs().max().item(),
            "pred_logits_max_abs_diff": (a["pred_logits"].float() - b["pred_logits"].float()).abs().max().item()}
    del a, b
    run(True), run(False)
    mo, ml, ml2 = timed([lambda: run(True), lambda: run(False), lambda: run(False)], iters)
    so, sl, sl2 = stats(mo), stats(ml), stats(ml2)
    emit({"part": "forward", "frames": T, "size": [H, W], "model": "config #2 (resnet101, 4+4 layers, 5 queries), initial weights, bf16 autocast, eval",
          "own": so, "library": sl, "library_again": sl2, "library_over_own_median": round(sl["median_ms"] / so["median_ms"], 4),
          "identical_runs_spread": round(abs(sl["median_ms"] - sl2["median_ms"]) / sl["median_ms"], 4), "entry_points_own": counts,
          "lfm_fallbacks_own": {k: v for k, v in fallbacks.snapshot().items() if k.startswith("LFM")}, **diff})
    modules.DFT_ANY = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfm_dft_any_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--forward-iters", type=int, default=6)
    ap.add_argument("--parts", default="block,sweep,forward")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lfm_dft_any_ab: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    modules.DFT_CZT = False           # this tool measures the plan stages and the direct stage; the chirp axis has tools/lfm_dft_czt_ab.py
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        parts = a.parts.split(",")
        if "block" in parts:
            block_ab(dev, a.iters, emit, (("train", TRAIN), ("eval", EVAL), ("old_served_neighbour", NEIGHBOUR)))
        if "sweep" in parts:
            block_ab(dev, a.iters, emit, (("sweep_w", [(10, 40, p) for p in SWEEP]), ("sweep_h", [(10, p, 40) for p in SWEEP]), ("sweep_long", LONG)))
        if "forward" in parts:
            forward_ab(dev, a.forward_iters, emit)


if __name__ == "__main__":
    main()
