"""fp32 against 16-bit-storage MSDeformAttn kernels at the config #2 encoder shape (N = 10, S = Lq = 5100, M = 8, D = 32, L = P = 4):
forward, gather half (grad_loc / grad_attn) and scatter half (grad_value) of the backward, in ONE process and alternating, warm
operands, HIP events around the C-ABI call only, on
  ring     the model's initial offsets,
  trained  ring + N(0, 3 px) + 5 % far outliers (the "trained-like" offsets of tools/bench_msda_gv.py).
The fused front end of the 16-bit path (ocpg_msda_fused_fwd_h16 / ocpg_msda_fused_bwd_qproj_h16: kernels "fwd_fused" / "gather_fused") is
timed in the same rounds, next to the un-fused 16-bit kernels it replaces, on the same locations and weights (qproj = [loc - ref | log attn]).
The 16-bit forward and gather run with 4 channels per lane (8-byte loads, variant a) and 8 (16-byte loads, variant b); at this shape
(D = 32, L * P = 16) the library honours both requests (for shapes whose records do not fit the LDS it serves 8 as 4).
--launches per kernel and round (default 200), --rounds (default 3: the spread over the rounds is the yardstick of "not slower").
Prints one JSON line per (offsets, kernel, variant) with the median microseconds of every round, the algorithmic bytes and the fraction
of 8 TB/s they amount to.  DTYPE=fp16 switches the 16-bit dtype (default bf16)."""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd._lib import lib, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=10)
a = ap.parse_args()

dev = torch.device("cuda:0")
shapes_l = [(48, 80), (24, 40), (12, 20), (6, 10)]
shapes = torch.tensor(shapes_l, dtype=torch.long)
S = int(shapes.prod(1).sum())
N, M, D, L, P = a.frames, 8, 32, 4, 4
h16 = torch.float16 if os.environ.get("DTYPE") == "fp16" else torch.bfloat16
code = 2 if h16 == torch.float16 else 1


def ring_loc(noise, outliers, seed=0):
    g = torch.Generator().manual_seed(seed)
    refs = []
    for (h, w) in shapes_l:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, w - 0.5, w) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, None, None, :]
    th = torch.arange(M) * (2 * math.pi / M)
    grid = torch.stack([th.cos(), th.sin()], -1)
    grid = grid / grid.abs().max(-1, keepdim=True)[0]
    off = (grid.view(1, 1, M, 1, 1, 2) * torch.arange(1, P + 1).view(1, 1, 1, 1, P, 1)).expand(N, S, M, L, P, 2)
    if noise:
        off = off + noise * torch.randn(N, S, M, L, P, 2, generator=g)
    norm = torch.tensor([[w, h] for h, w in shapes_l], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = (ref + off / norm).contiguous()
    if outliers:
        far = torch.rand(N, S, M, L, P, 1, generator=g) < outliers
        loc = torch.where(far, torch.rand(N, S, M, L, P, 2, generator=g) * 1.2 - 0.1, loc)
    return loc.contiguous()


g = torch.Generator().manual_seed(1)
attn = torch.softmax(torch.randn(N, S, M, L * P, generator=g), -1).view(N, S, M, L, P).to(dev)
v32 = torch.randn(N, S, M, D, generator=g).to(dev)
go32 = torch.randn(N, S, M * D, generator=g).to(dev)
v16, go16 = v32.to(h16), go32.to(h16)
out32, out16 = torch.empty_like(go32), torch.empty_like(go16)
gv = torch.zeros(N, S, M, D, device=dev)
ds = shapes.to(dev)
dls = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1])).to(dev)
hs = ctypes.c_void_p(shapes.data_ptr())
dims = (N, S, M, D, L, S, P)
n_val, n_samp = N * S * M * D, N * S * M * L * P
BYTES = {   # algorithmic: every operand once
    ("fwd", 4): 4 * n_val + 12 * n_samp + 4 * n_val, ("fwd", 2): 2 * n_val + 12 * n_samp + 2 * n_val,
    ("gather", 4): 4 * n_val + 12 * n_samp + 4 * n_val + 12 * n_samp, ("gather", 2): 2 * n_val + 12 * n_samp + 2 * n_val + 12 * n_samp,
    ("scatter", 4): 12 * n_samp + 4 * n_val + 4 * n_val, ("scatter", 2): 12 * n_samp + 2 * n_val + 4 * n_val,
    # fused front end: value + out + qproj read + loc / attn written + ref;  value + loc / attn + grad_out read + grad_qproj written
    ("fwd_fused", 2): 2 * n_val + 2 * n_val + 12 * n_samp + 12 * n_samp + 4 * N * S * L * 2,
    ("gather_fused", 2): 2 * n_val + 12 * n_samp + 2 * n_val + 12 * n_samp,
}


def calls(loc):
    gl, ga = torch.empty_like(loc), torch.empty_like(attn)
    # the fused front end's inputs for the same samples: every query's own pixel centre as reference point on every level
    refs = []
    for (h, w) in shapes_l:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, w - 0.5, w) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, L, 2).contiguous().to(dev)
    qproj = torch.cat([(loc - ref[:, :, None, :, None, :]).reshape(N, S, -1), attn.log().reshape(N, S, -1)], -1).contiguous()
    loc_o, attn_o, gq = torch.empty_like(loc), torch.empty_like(attn), torch.empty_like(qproj)
    L_ = lib()
    p = lambda t: t.data_ptr()
    return {
        ("fwd", "fp32"): lambda: L_.ocpg_msda_fwd_f32(p(v32), p(ds), p(dls), p(loc), p(attn), *dims, p(out32), None, stream_ptr()),
        ("fwd", "h16"): lambda: L_.ocpg_msda_fwd_h16(p(v16), p(ds), p(dls), p(loc), p(attn), *dims, p(out16), None, code, stream_ptr()),
        ("gather", "fp32"): lambda: L_.ocpg_msda_bwd_locattn_f32(p(v32), p(ds), p(dls), p(loc), p(attn), p(go32), *dims, p(gl), p(ga), stream_ptr()),
        ("gather", "h16"): lambda: L_.ocpg_msda_bwd_locattn_h16(p(v16), p(ds), p(dls), p(loc), p(attn), p(go16), *dims, p(gl), p(ga), code, stream_ptr()),
        ("fwd_fused", "h16"): lambda: L_.ocpg_msda_fused_fwd_h16(p(v16), p(ds), p(dls), p(qproj), p(ref), *dims, p(out16), p(loc_o), p(attn_o), code,
                                                                 stream_ptr()),
        ("gather_fused", "h16"): lambda: L_.ocpg_msda_fused_bwd_qproj_h16(p(v16), p(ds), p(dls), p(loc), p(attn), p(go16), *dims, p(gq), code, stream_ptr()),
        ("scatter", "fp32"): lambda: L_.ocpg_msda_bwd_value_f32(p(loc), p(attn), p(go32), *dims, p(gv), hs, stream_ptr()),
        ("scatter", "h16"): lambda: L_.ocpg_msda_bwd_value_h16(p(loc), p(attn), p(go16), *dims, p(gv), hs, None, code, stream_ptr()),
    }, (gl, ga, ref, qproj, loc_o, attn_o, gq)


def timed(fn, n, zero):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        if zero:
            gv.zero_()
        e0.record()
        rc = fn()
        e1.record()
        assert rc == 0, rc
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[n // 2]


VARIANTS = [("fwd", "fp32", None), ("fwd", "h16", "4"), ("fwd_fused", "h16", "4"), ("fwd", "h16", "8"), ("fwd_fused", "h16", "8"),
            ("gather", "fp32", None), ("gather", "h16", "4"), ("gather_fused", "h16", "4"), ("gather", "h16", "8"), ("gather_fused", "h16", "8"),
            ("scatter", "fp32", None), ("scatter", "h16", None)]
for mode, noise, outl in (("ring", 0.0, 0.0), ("trained", 3.0, 0.05)):
    loc = ring_loc(noise, outl).to(dev)
    fns, keep = calls(loc)
    res = {v: [] for v in VARIANTS}
    for rnd in range(a.rounds + 1):                 # round 0 warms up (code objects, caches) and is dropped
        for v in VARIANTS:                          # alternating: every variant once per round
            kern, kind, lanes = v
            if lanes is not None:
                os.environ["OCPG_MSDA_H16_LANES"] = lanes
            us = timed(fns[(kern, kind)], a.launches if rnd else 20, kern == "scatter")
            os.environ.pop("OCPG_MSDA_H16_LANES", None)
            if rnd:
                res[v].append(round(us, 1))
    for (kern, kind, lanes), us in res.items():
        b = BYTES[(kern, 4 if kind == "fp32" else 2)]
        med = sorted(us)[len(us) // 2]
        print(json.dumps({"offsets": mode, "kernel": kern, "storage": "fp32" if kind == "fp32" else str(h16).replace("torch.", ""),
                          "channels_per_lane": int(lanes) if lanes else (4 if kind == "fp32" or kern != "scatter" else None),
                          "us_rounds": us, "us": med, "algorithmic_MB": round(b / 1e6, 1), "fraction_of_8TBps": round(b / (med * 1e-6) / 8e12, 3),
                          "launches_per_round": a.launches, "frames": N}), flush=True)
