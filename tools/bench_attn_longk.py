"""The long-key attention kernels (csrc/attn_longk.hip) against the library path they replace, for the SAME MultiheadAttention module:

  new  OCPG_ATTN_LONGK=force: amp_cache.linear projections + ocpg_attn_longk_fwd / _bwd on the [L, B, C] rows (force: also past the
                              default bound attn_smallk_func.MAX_KEYS, which these lines decide)
  lib  OCPG_ATTN_LONGK=0:     F.linear projections, head permutes, additive mask, F.scaled_dot_product_attention (what served more
                              than 32 keys before the kernels existed)

forward + backward (gradients of the inputs and of every parameter) under bf16 autocast, at the text gate's shape of config #2's
largest level (Lq = 19 200, B = 2, H = 8; Lk in {40, 64, 128}, the second caption padded to 12 tokens) and at a many-query decoder
self-attention (Lq = Lk = 50, B = 10, dropout 0.1).  Both paths alternate in ONE process; HIP events around each call; median of
3 rounds x 30 calls, back to back ("warm") and with 1 GiB written between calls ("cold": what a training step looks like to these
kernels).  One JSON line per shape, with the long-key kernels' own times (events around the two library calls) next to it.

    python tools/bench_attn_longk.py > profiles/attn_longk_bench.jsonl"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd import _lib
from ocpg_amd.models.attention import MultiheadAttention

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

dev = torch.device("cuda:0")
C, H = 256, 8
g = torch.Generator().manual_seed(1)
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)          # 1 GiB


def case(name, Lq, B, Lk, self_attn, dropout):
    m = MultiheadAttention(C, H, dropout=dropout).to(dev).train()
    q = torch.randn(Lq, B, C, generator=g).to(dev).requires_grad_(True)
    if self_attn:
        k, v, pad = q, torch.randn(Lk, B, C, generator=g).to(dev).requires_grad_(True), None
    else:
        k = torch.randn(Lk, B, C, generator=g).to(dev).requires_grad_(True)
        v = torch.randn(Lk, B, C, generator=g).to(dev).requires_grad_(True)
        pad = torch.zeros(B, Lk, dtype=torch.bool, device=dev)
        pad[1, 12:] = True                                              # one long caption pads the other
    go = torch.randn(Lq, B, C, generator=g).to(dev)
    leaves = [q, v] + ([] if self_attn else [k]) + list(m.parameters())

    def call():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(q, k, v, key_padding_mask=pad)
        return torch.autograd.grad(out.float(), leaves, go)
    return name, (Lq, B, H, Lk), call


def run(fn, mode):
    os.environ["OCPG_ATTN_LONGK"] = "0" if mode == "lib" else "force"
    try:
        return fn()
    finally:
        os.environ.pop("OCPG_ATTN_LONGK", None)


def timed(fn, mode, n, cold):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        if cold:
            flush.fill_(1.0)
        e0.record()
        run(fn, mode)
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[n // 2]


warnings.simplefilter("ignore", RuntimeWarning)                         # the library path is a counted fallback and says so
cases = [case(f"fusion Lk={lk}", 19200, 2, lk, False, 0.0) for lk in (40, 64, 128)] + [case("decoder 50 queries", 50, 10, 50, True, 0.1)]
for name, shape, fn in cases:
    res = {(k, m): [] for k in ("lib", "new") for m in ("warm", "cold")}
    for rnd in range(a.rounds + 1):                 # round 0 warms up (code objects, GEMM plans) and is dropped
        for m in ("warm", "cold"):
            for k in ("lib", "new"):                # alternating: every path once per round and mode
                us = timed(fn, k, a.calls if rnd else 5, m == "cold")
                if rnd:
                    res[(k, m)].append(round(us, 1))
    med = {km: sorted(v)[len(v) // 2] for km, v in res.items()}
    kern = {}
    for cold in (False, True):                      # the kernels alone: events around the two C-ABI calls
        _lib.enable_kernel_timing(True)
        for _ in range(10):
            if cold:
                flush.fill_(1.0)
            run(fn, "new")
        t = _lib.collect_kernel_timing()
        for sym in ("ocpg_attn_longk_fwd", "ocpg_attn_longk_bwd"):
            kern[f"{sym[10:]}_{'cold' if cold else 'warm'}_us"] = round(t[sym]["ms"] / t[sym]["n"] * 1e3, 1)
    print(json.dumps({"case": name, "Lq_B_H_Lk": shape, "dtype": "bf16",
                      "lib_warm_us": med[("lib", "warm")], "new_warm_us": med[("new", "warm")],
                      "lib_cold_us": med[("lib", "cold")], "new_cold_us": med[("new", "cold")],
                      "speedup_warm": round(med[("lib", "warm")] / med[("new", "warm")], 2),
                      "speedup_cold": round(med[("lib", "cold")] / med[("new", "cold")], 2),
                      "kernels": kern, "rounds_us": {f"{k}_{m}": v for (k, m), v in res.items()}, "calls_per_round": a.calls}), flush=True)
