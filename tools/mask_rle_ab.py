"""A/B of the run-length encoder on the device (csrc/mask_rle.hip through models/ops/functions/mask_rle_func.py) against the host
loop it stands in for, on one GPU, in one process, the legs alternated call by call, each call between its own pair of device events
(a call's host work -- tables, readbacks, the Python loop -- lies between them as well).

Inputs, each at two run densities (`smooth` blobs, `rough` randn x 8; tests/mask_tail_ref.py's generator on the stride-4 map, nearest
x4 as the model's eval branch makes `pred_masks`):
  a2d     one batch of an A2D-Sentences evaluation at the 320-pixel short side: B = 2, Q = 5, 320 x 428 and 320 x 568 padded to 320 x 576
  720p    one sample of 5 queries at 720 x 1280

Legs:
  host          A2DSentencesPostProcess(native=False): the chain, Q planes to the host, the Python loop (the parent's path)
  planes        A2DSentencesPostProcess(native=True): the same chain, the planes encoded on the device
  planes_again  the same leg once more per round: the difference of the two medians is the spread of identical runs
  logits        rle_from_logits alone: no plane at the original resolution at all
  pack / encode the two C entries of the logits form by themselves, tables and buffers made beforehand (pass 1 + totals; passes 2 + 3)
`planes_wins` / `logits_wins` count the rounds in which the leg beat `host` by more than the spread.  One JSON line per input.

--kernels-only runs the 720p inputs a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for
per-kernel times; --kernel-stats DB appends the rle_* kernels of that run's database (its `kernels` view) to the output file.
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
from ocpg_amd._lib import lib, stream_ptr
from ocpg_amd.models.ops.functions.mask_rle_func import rle_area, rle_from_logits, workspace_bytes
from ocpg_amd.models.postprocessors import A2DSentencesPostProcess

Q = 5
INPUTS = {"a2d": ((320, 576), [(320, 428), (320, 568)]), "720p": ((720, 1280), [(720, 1280)])}


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


def make(name, kind, dev):
    padded, sizes = INPUTS[name]
    b = len(sizes)
    low = mask_tail_ref.logits((b * Q, padded[0] // 4, padded[1] // 4), kind, 7).view(b, Q, padded[0] // 4, padded[1] // 4).to(dev)
    return F.interpolate(low, scale_factor=4), sizes


def raw_entries(full, sizes, dev):
    """The two C entries of the logits form on buffers made beforehand -> (pack, encode) callables."""
    L = lib()
    b, q, hs, ws = full.shape
    n = b * q
    geom = torch.tensor([list(s) + list(s) for s in sizes], dtype=torch.int32)
    geom_dev = geom.to(dev)
    max_n = max(h * w for h, w in sizes)
    work = torch.empty(workspace_bytes(n, max_n), dtype=torch.uint8, device=dev)
    n_trans = torch.empty(n, dtype=torch.int32, device=dev)

    def pack():
        return L.ocpg_mask_rle_pack_logits_f32(full.data_ptr(), b, q, hs, ws, 1, geom.data_ptr(), geom_dev.data_ptr(), max_n, 0.5, 1,
                                               n_trans.data_ptr(), work.data_ptr(), stream_ptr())
    assert pack() == 0
    nt = n_trans.cpu()
    start = torch.zeros(n, dtype=torch.int64)
    start[1:] = torch.cumsum(nt[:-1].long() + 1, 0)
    cap = int(start[-1]) + int(nt[-1]) + 1
    start_dev = start.to(dev)
    counts = torch.empty(cap, dtype=torch.int32, device=dev)
    n_runs = torch.empty(n, dtype=torch.int32, device=dev)
    text = torch.empty(7 * cap, dtype=torch.uint8, device=dev)
    n_bytes = torch.empty(n, dtype=torch.int64, device=dev)

    def encode():
        return L.ocpg_mask_rle_encode(n, max_n, nt.data_ptr(), start.data_ptr(), start_dev.data_ptr(), cap, counts.data_ptr(), n_runs.data_ptr(),
                                      text.data_ptr(), n_bytes.data_ptr(), work.data_ptr(), stream_ptr())
    assert encode() == 0
    return pack, encode, cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_rle_ab.jsonl"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        import re
        import sqlite3
        rows = sqlite3.connect(args.kernel_stats).execute("select name, duration from kernels where name like '%rle_%'").fetchall()
        per = {}
        for name, ns in rows:
            per.setdefault(re.search(r"rle_\w+", name).group(0), []).append(ns / 1e3)
        d = {"kernel_us_720p_smooth_and_rough": {k: {"calls": len(v), "median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                                     "max": round(max(v), 2)} for k, v in per.items()}}
        print(json.dumps(d))
        with open(args.out, "a") as f:
            f.write(json.dumps(d) + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("mask_rle_ab.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    if args.kernels_only:
        for kind in ("smooth", "rough"):
            full, sizes = make("720p", kind, dev)
            out = {"pred_logits": torch.zeros(1, 1, Q, 1, device=dev), "pred_masks": full[:, None]}
            for _ in range(5):
                rle_from_logits(full, 1, sizes, sizes, native=True)
                A2DSentencesPostProcess(native=True)(out, torch.tensor(sizes), torch.tensor(sizes))
        torch.cuda.synchronize()
        return
    lines = []
    for name in INPUTS:
        for kind in ("smooth", "rough"):
            full, sizes = make(name, kind, dev)
            b = len(sizes)
            outputs = {"pred_logits": torch.randn(b, 1, Q, 1, generator=torch.Generator().manual_seed(0)).to(dev), "pred_masks": full[:, None]}
            orig = size = torch.tensor(sizes)
            host_post, dev_post = A2DSentencesPostProcess(native=False), A2DSentencesPostProcess(native=True)

            def host():
                return host_post(outputs, orig, size)

            def planes():
                return dev_post(outputs, orig, size)

            def logits():
                return rle_from_logits(full, 1, sizes, sizes, native=True)
            pack, encode, cap = raw_entries(full, sizes, dev)
            want, got, fused = host(), planes(), logits()
            same = all(w["rle_masks"] == g["rle_masks"] for w, g in zip(want, got))
            differ = sum(abs(rle_area(a) - rle_area(c)) for w, f in zip(want, fused) for a, c in zip(w["rle_masks"], f))
            for _ in range(2):
                host(), planes(), logits(), pack(), encode()
            mh, mp, mp2, ml, mk, me = timed([host, planes, planes, logits, pack, encode], args.iters)
            sh, sp, sp2, sl, sk, se = (stats(x) for x in (mh, mp, mp2, ml, mk, me))
            spread = abs(sp["median_ms"] - sp2["median_ms"]) / min(sp["median_ms"], sp2["median_ms"])
            d = {"input": name, "kind": kind, "queries": Q, "sizes": sizes, "runs": cap,
                 "string_bytes": sum(len(r["counts"]) for w in want for r in w["rle_masks"]),
                 "host": sh, "planes": sp, "planes_again": sp2, "logits": sl, "pack": sk, "encode": se,
                 "identical_runs_spread": round(spread, 4),
                 "planes_wins": sum(p * (1 + spread) < h for p, h in zip(mp, mh)), "logits_wins": sum(x * (1 + spread) < h for x, h in zip(ml, mh)),
                 "rounds": args.iters, "host_over_planes": round(sh["median_ms"] / sp["median_ms"], 2),
                 "host_over_logits": round(sh["median_ms"] / sl["median_ms"], 2),
                 "planes_strings_equal_host": same, "logits_area_difference_to_host_pixels": differ,
                 "device": torch.cuda.get_device_name(0)}
            print(json.dumps(d), flush=True)
            lines.append(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
