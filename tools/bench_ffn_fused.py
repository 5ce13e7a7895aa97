"""The encoder FFN's two GEMM + memory-pass pairs against their fused forms (csrc/gemm_dgrad_bn.hip) at the encoder's shapes:
M = 51 000 / 25 500 rows (2 clips / 1 clip), N = 2048, K = 256, bf16.  HIP events around the C-ABI calls, median of 30; every variant is
timed cold (1 GiB written between calls) and warm, alternated in one process.  One JSON line per (direction, M, cold):

  bwd  pair  = ocpg_gemm (linear2's input gradient) + ocpg_bias_relu_dropout_bwd
       bn    = ocpg_gemm_dgrad_bn with c = NULL, mask = h and a constant scale vector, its three tiles (no column sums: the arithmetic only)
       fused = ocpg_gemm_dgrad_mask, its three tiles (with the partial column sums)
  fwd  pair  = ocpg_gemm (linear1) + ocpg_bias_relu_dropout_fwd
       fused = ocpg_gemm_bias_relu_dropout_fwd (round_gemm = 1, the pair's arithmetic: what the step runs), its three tiles

    python tools/bench_ffn_fused.py > profiles/ffn_fused_kernel_level.jsonl"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd._lib import lib, stream_ptr

N, K, P = 2048, 256, 0.1
TILES = ("128x128", "64x128", "64x64")
TILE_ROWS = (128, 64, 64)
dev = torch.device("cuda:0")
cold_buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)
L = lib()


def timed(fn, cold, n=30):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        if cold:
            cold_buf.fill_(1.0)
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return round(sorted(a.elapsed_time(b) * 1e3 for a, b in ev)[n // 2], 1)


for m in (51000, 25500):
    g = torch.Generator().manual_seed(0)
    bf = torch.bfloat16
    x = torch.randn(m, K, generator=g).to(dev, bf)                      # linear1's input / the gradient at linear2's output
    w1 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, bf)        # linear1.weight [N][K]
    w2 = (torch.randn(K, N, generator=g) / N ** 0.5).to(dev, bf)        # linear2.weight [K][N]
    b1 = torch.randn(N, generator=g).to(dev, bf)
    h, h2, gv, ga = (torch.empty(m, N, dtype=bf, device=dev) for _ in range(4))
    ones = torch.full((N,), 1.0 / (1.0 - P), device=dev)
    slots = int(L.ocpg_bias_relu_dropout_bwd_slots(m, N, 1))
    part_pair = torch.empty(slots, N, device=dev)
    part = torch.empty((m + 63) // 64, N, device=dev)
    st = stream_ptr()
    p = lambda t: t.data_ptr()      # noqa: E731

    def fwd_pair():
        assert L.ocpg_gemm(p(x), p(w1), p(h), None, 1, 1, 0, 1, m, N, K, K, K, N, 1, 0, 0, 0, 1.0, 0.0, st) == 0
        assert L.ocpg_bias_relu_dropout_fwd(p(h), p(b1), m, N, P, 7, 3, None, 1, p(h), st) == 0

    def fwd_fused(t):
        assert L.ocpg_gemm_bias_relu_dropout_fwd(p(x), p(w1), p(b1), P, 7, 3, None, p(h2), m, N, K, 1, t, 1, st) == 0

    def bwd_pair():
        assert L.ocpg_gemm(p(x), p(w2), p(gv), None, 1, 1, 0, 0, m, N, K, K, N, N, 1, 0, 0, 0, 1.0, 0.0, st) == 0
        assert L.ocpg_bias_relu_dropout_bwd(p(gv), p(h), m, N, P, 1, p(ga), p(part_pair), st) == 0

    def bwd_bn(t):
        assert L.ocpg_gemm_dgrad_bn(p(x), p(w2), None, p(h), p(ones), p(h2), None, m, N, K, 1, t, st) == 0

    def bwd_fused(t):
        assert L.ocpg_gemm_dgrad_mask(p(x), p(w2), p(h), 1.0 / (1.0 - P), p(h2), p(part), m, N, K, 1, t, st) == 0

    # the fused results against the pairs on the same inputs (norm-relative; the pair rounds once more)
    fwd_pair(); fwd_fused(0)
    torch.cuda.synchronize()
    same_mask = bool(torch.equal(h == 0, h2 == 0))
    err_f = ((h2.float() - h.float()).norm() / h.float().norm()).item()
    bwd_pair(); bwd_fused(0)
    torch.cuda.synchronize()
    err_b = ((h2.float() - ga.float()).norm() / ga.float().norm()).item()
    err_cs = ((part[:(m + 127) // 128].sum(0) - part_pair.sum(0)).norm() / part_pair.sum(0).norm()).item()
    for _ in range(2):                      # alternated: cold, warm, cold, warm ("rep" 0 / 1: the run-to-run spread inside the process)
        for cold in (True, False):
            print(json.dumps({"dir": "fwd", "M": m, "N": N, "K": K, "cold": cold, "rep": _, "pair_us": timed(fwd_pair, cold),
                              "fused_us": {TILES[t]: timed(lambda: fwd_fused(t), cold) for t in range(3)},
                              "rel_diff_vs_pair": round(err_f, 5), "same_zero_pattern": same_mask}), flush=True)
            print(json.dumps({"dir": "bwd", "M": m, "N": N, "K": K, "cold": cold, "rep": _, "pair_us": timed(bwd_pair, cold),
                              "dgrad_bn_us": {TILES[t]: timed(lambda: bwd_bn(t), cold) for t in range(3)},
                              "fused_us": {TILES[t]: timed(lambda: bwd_fused(t), cold) for t in range(3)},
                              "rel_diff_vs_pair": round(err_b, 5), "colsum_rel_diff_vs_pair": round(err_cs, 6)}), flush=True)
