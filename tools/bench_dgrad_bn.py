"""ocpg_gemm_dgrad_bn (1x1 input gradient + the frozen-BN / ReLU backward of the layer in front, csrc/gemm_dgrad_bn.hip) against the pair it
replaces (ocpg_gemm input gradient + ocpg_bn_act_bwd) at the ResNet-101 body's site shapes, 2 and 1 clips of 10 frames.  HIP events
around the C-ABI calls, median of 30; BN_COLD=1 writes 1 GiB between calls.  One JSON line per shape: the pair and the fused kernel at the
tile ocpg_gemm_dgrad_bn_tile picks (and at every other tile, "by_tile"), TFLOP/s against 2.5 PF, GB/s of the fused kernel's byte floor
against 8 TB/s, and which bound is the larger.
Site (a): conv3's input gradient, out = bf16(v [x > 0] scale2);  site (b): conv1's, C = the parked skip gradient, out_skip = bf16(m),
out = bf16(m scale3), m = (v + C) [x > 0].
--dtype bf16 (default) | fp16 | both: the storage type (C-ABI dtype code 1 / 2).  `both` times every shape as bf16, fp16, bf16 in that
order ("rep" 0 / 1 in the line): the two bf16 figures of one call are the run-to-run spread the fp16 figure is read against."""
import argparse
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd._lib import lib, stream_ptr

PEAK_FLOPS, PEAK_BW = 2.5e15, 8e12
SITES = (("a", "L2", 38400, 128, 512), ("a", "L3", 9600, 256, 1024), ("a", "L4", 2400, 512, 2048),
         ("b", "L2", 38400, 512, 128), ("b", "L3", 9600, 1024, 256), ("b", "L4", 2400, 2048, 512))
dev = torch.device("cuda:0")
cold_buf = torch.empty(1 << 28, dtype=torch.float32, device=dev) if os.environ.get("BN_COLD") == "1" else None
L = lib()
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("bf16", "fp16", "both"), default="bf16")
ARGS = ap.parse_args()
RUNS = {"bf16": (("bf16", 0),), "fp16": (("fp16", 0),), "both": (("bf16", 0), ("fp16", 0), ("bf16", 1))}[ARGS.dtype]
TORCH_DT = {"bf16": (torch.bfloat16, 1), "fp16": (torch.float16, 2)}


def timed(fn, n=30):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        if cold_buf is not None:
            cold_buf.fill_(1.0)
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)[n // 2]


for site, layer, m2, n, k in SITES:
    for clips, (dname, rep_i) in itertools.product((2, 1), RUNS):
        tdt, code = TORCH_DT[dname]
        m = m2 * clips // 2
        g = torch.Generator().manual_seed(0)
        a = torch.randn(m, k, generator=g).to(dev, tdt)                 # gz of the consumer
        w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev, tdt)    # its weight [Cout][Cin]
        x = torch.randn(m, n, generator=g).to(dev, tdt)                 # its input = the mask
        scale = (torch.rand(n, generator=g) + 0.5).to(dev)
        c = torch.randn(m, n, generator=g).to(dev, tdt) if site == "b" else None
        gx, gz, gskip = (torch.empty(m, n, dtype=tdt, device=dev) for _ in range(3))
        tile = int(L.ocpg_gemm_dgrad_bn_tile(m, n, k))
        st = stream_ptr()

        def old():          # what conv_bn_func ran before: hipBLASLt dgrad (beta = 1 onto C at site b), then the BN / ReLU backward
            dst = c if c is not None else gx
            assert L.ocpg_gemm(a.data_ptr(), w.data_ptr(), dst.data_ptr(), None, code, code, 0, 0, m, n, k, k, n, n, 1, 0, 0, 0, 1.0,
                               1.0 if c is not None else 0.0, st) == 0
            assert L.ocpg_bn_act_bwd(dst.data_ptr(), x.data_ptr(), scale.data_ptr(), gz.data_ptr(), gskip.data_ptr() if c is not None else None,
                                     m, n, 1, 1, code, st) == 0

        def new(t=tile):
            assert L.ocpg_gemm_dgrad_bn(a.data_ptr(), w.data_ptr(), None if c is None else c.data_ptr(), x.data_ptr(), scale.data_ptr(),
                                        gz.data_ptr(), None if c is None else c.data_ptr(), m, n, k, code, t, st) == 0

        # the fused result against the pair on the same inputs (C is updated in place by both: compare from a fresh copy)
        c0 = None if c is None else c.clone()
        old()
        ref = gz.float().clone()
        if c is not None:
            c.copy_(c0)
        new()
        torch.cuda.synchronize()
        err = ((gz.float() - ref).norm() / ref.norm()).item()
        t_old, t_new = timed(old), timed(new)
        by_tile = {("128x128", "64x128", "64x64")[t]: round(timed(lambda: new(t)), 1) for t in range(3)}
        flops = 2.0 * m * n * k
        byt = 2.0 * (m * k + k * n + m * n * (2 if c is None else 4))           # A + W + mask (+ C) + outputs
        t_floor = max(flops / PEAK_FLOPS, byt / PEAK_BW) * 1e6
        print(json.dumps({"dtype": dname, "rep": rep_i, "site": site, "layer": layer, "clips": clips, "M": m, "N": n, "K": k, "tile": ("128x128", "64x128", "64x64")[tile],
                          "cold": cold_buf is not None, "old_pair_us": round(t_old, 1), "fused_us": round(t_new, 1),
                          "speedup": round(t_old / t_new, 2), "fused_TFLOPs": round(flops / t_new / 1e6, 1),
                          "frac_of_2.5PF": round(flops / t_new / 1e6 / 2500, 3), "fused_GBs": round(byt / t_new / 1e3, 1),
                          "frac_of_8TBs": round(byt / t_new / 1e3 / 8000, 3),
                          "bound": "hbm" if byt / PEAK_BW > flops / PEAK_FLOPS else "mfma", "floor_us": round(t_floor, 1),
                          "rel_err_vs_pair": round(err, 5), "by_tile_us": by_tile}), flush=True)
