"""ocpg_conv3x3_mfma_wgrad (csrc/conv3x3_wgrad_kernel.h) against its ring form ocpg_conv3x3_mfma_wgrad_ring (csrc/conv3x3_wgrad_ring_kernel.h)
at the four ResNet-101 shapes of tools/bench_wgrad.py (config #2, 10 frames), alternately in ONE process: HIP events around each C-ABI call,
warm (back to back) and cold (1 GiB written between calls), the median of 30 calls, two repetitions.  One JSON line per shape and mode;
"ring" is null where the entry point declines the shape (-2000).  The two results are compared bit for bit first (WG_NOCHECK=1: not, for a
phase-cut build of the library, -DWG_CUT_LOAD / -DWG_CUT_COMPUTE, named by OCPG_HIP_LIB).  `--out FILE` appends the lines to FILE as well."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd._lib import lib, check

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=30)
ARGS = ap.parse_args()
dev = torch.device("cuda:0")
L = lib()
cold_buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)
SHAPES = {"layer2 (128, 48x80)": (10, 128, 128, 48, 80, 1), "layer3 (256, 24x40)": (10, 256, 256, 24, 40, 1),
          "layer4 (512, 12x20)": (10, 512, 512, 12, 20, 1), "layer3.0 stride 2": (10, 256, 256, 48, 80, 2)}


def times(fns, cold, calls):
    """-> {name: [us per call]}: the functions called alternately, each call between its own pair of events"""
    out = {k: [] for k in fns}
    for k, fn in fns.items():           # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    pairs = []
    for _ in range(calls):
        for k, fn in fns.items():
            if cold:
                cold_buf.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs.append((k, e0, e1))
    torch.cuda.synchronize()
    for k, e0, e1 in pairs:
        out[k].append(e0.elapsed_time(e1) * 1e3)
    return out


for name, (n, c, co, h, w, s) in SHAPES.items():
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    x = torch.randn(n, h, w, c, device=dev).to(torch.bfloat16)
    gz = torch.randn(n, ho, wo, co, device=dev).to(torch.bfloat16)
    sp = int(L.ocpg_conv3x3_mfma_wgrad_splits(n, h, w, c, co, s))
    part, part_r = (torch.empty(sp, co, 9 * c, device=dev, dtype=torch.bfloat16) for _ in range(2))
    st = torch.cuda.current_stream().cuda_stream
    a = (gz.data_ptr(), x.data_ptr(), n, h, w, c, co, s)
    fns = {"present": lambda: check(L.ocpg_conv3x3_mfma_wgrad(*a, part.data_ptr(), st), "ocpg_conv3x3_mfma_wgrad")}
    rc = L.ocpg_conv3x3_mfma_wgrad_ring(*a, part_r.data_ptr(), st)
    if rc != -2000:
        check(rc, "ocpg_conv3x3_mfma_wgrad_ring")
        fns["present"]()
        torch.cuda.synchronize()
        assert os.environ.get("WG_NOCHECK") == "1" or torch.equal(part.view(torch.int16), part_r.view(torch.int16)), name
        fns["ring"] = lambda: check(L.ocpg_conv3x3_mfma_wgrad_ring(*a, part_r.data_ptr(), st), "ocpg_conv3x3_mfma_wgrad_ring")
    fl = 2.0 * n * ho * wo * co * 9 * c
    for cold in (0, 1):
        for rep in range(2):
            t = times(fns, cold, ARGS.calls)
            rec = {"shape": name, "splits": sp, "cold": cold, "rep": rep, "calls": ARGS.calls}
            for k in ("present", "ring"):
                rec[k] = None if k not in t else {"median_us": round(statistics.median(t[k]), 2), "min_us": round(min(t[k]), 2),
                                                  "tflops": round(fl / statistics.median(t[k]) / 1e6, 1)}
            line = json.dumps(rec)
            print(line, flush=True)
            if ARGS.out:
                with open(ARGS.out, "a") as f:
                    f.write(line + "\n")
