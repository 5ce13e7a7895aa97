"""Today's cross-attention value path against the sample-first kernels (csrc/msda_sample_first.hip) at the config #2 decoder shape
(N = 10, S = 5100, M = 8, D = 32, L = P = 4) for Lq in {1, 5, 20, 50, 100, 300}:

  old  amp_cache.linear(src, Wv, bv) -> masked_fill(pad) -> MSDeformAttnFunction, and its backward (grad of src, Wv, bv, loc, attn)
  new  MSDeformAttnSampleFirstFunction, and its backward (the same five gradients)

in ONE process and alternating, HIP events around forward + backward, both back to back ("warm") and with 1 GiB written between calls
("cold": what a training step looks like to these kernels -- none of their operands is in a cache when they start).
One JSON line per Lq: median microseconds per variant and mode, the ratio, and 4*Lq*L*P / S (what `sample_first_wanted` compares to r).

    python tools/bench_msda_sample_first.py > profiles/msda_sample_first_kernel_level.jsonl"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd.models import amp_cache
from ocpg_amd.models.ops.functions import MSDeformAttnFunction
from ocpg_amd.models.ops.functions.ms_deform_attn_func import MSDeformAttnSampleFirstFunction

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--queries", type=int, nargs="*", default=[1, 5, 20, 50, 100, 300])
a = ap.parse_args()

dev = torch.device("cuda:0")
shapes_l = [(48, 80), (24, 40), (12, 20), (6, 10)]
shapes = torch.tensor(shapes_l, dtype=torch.long)
S = int(shapes.prod(1).sum())
N, M, D, L, P = a.frames, 8, 32, 4, 4
C = M * D
g = torch.Generator().manual_seed(1)
ds = shapes.to(dev)
dls = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1])).to(dev)
src = torch.randn(N, S, C, generator=g).to(dev).requires_grad_(True)
wv = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev).requires_grad_(True)
bv = torch.randn(C, generator=g).to(dev).requires_grad_(True)
pad = torch.zeros(N, S, dtype=torch.bool, device=dev)
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)          # 1 GiB


def variants(Lq):
    loc = (torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.1 - 0.05).to(dev).requires_grad_(True)
    attn = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).to(dev).requires_grad_(True)
    go = torch.randn(N, Lq, C, generator=g).to(dev)
    leaves = [src, wv, bv, loc, attn]

    def old():
        value = amp_cache.linear(src, wv, bv).masked_fill(pad[..., None], 0.0).view(N, S, M, D)
        out = MSDeformAttnFunction.apply(value, ds, dls, loc, attn, 64)
        return torch.autograd.grad(out, leaves, go)

    def new():
        out = MSDeformAttnSampleFirstFunction.apply(src, wv, bv, pad, ds, dls, loc, attn)
        return torch.autograd.grad(out, leaves, go)
    return {"old": old, "new": new}


def timed(fn, n, cold):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        if cold:
            flush.fill_(1.0)
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[n // 2]


for Lq in a.queries:
    fns = variants(Lq)
    res = {(k, m): [] for k in fns for m in ("warm", "cold")}
    for rnd in range(a.rounds + 1):                 # round 0 warms up (code objects, GEMM plans) and is dropped
        for m in ("warm", "cold"):
            for k, fn in fns.items():               # alternating: every variant once per round and mode
                us = timed(fn, a.calls if rnd else 5, m == "cold")
                if rnd:
                    res[(k, m)].append(round(us, 1))
    med = {km: sorted(v)[len(v) // 2] for km, v in res.items()}
    print(json.dumps({"Lq": Lq, "frames": N, "S": S, "ratio_4LqLP_over_S": round(4 * Lq * L * P / S, 4),
                      "old_warm_us": med[("old", "warm")], "new_warm_us": med[("new", "warm")],
                      "old_cold_us": med[("old", "cold")], "new_cold_us": med[("new", "cold")],
                      "speedup_warm": round(med[("old", "warm")] / med[("new", "warm")], 2),
                      "speedup_cold": round(med[("old", "cold")] / med[("new", "cold")], 2),
                      "rounds_us": {f"{k}_{m}": v for (k, m), v in res.items()}, "calls_per_round": a.calls}), flush=True)
