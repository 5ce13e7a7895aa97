"""Micro-benchmark of the window-attention BACKWARD with the relative-position table as the differentiable input: the default path
(`window_attention` + `RelPosBias`: k_bwd_q stores dS, ATen sums it over the windows, relpos_bias_bwd folds the sum into the table)
against the opt-in fused one (`window_attention_table`: k_bwd_q_dtable sums in LDS, k_dtable_reduce adds the windows).

Per shape and path: the backward alone, back to back (`--iters` calls between two events) and cold (a 1 GiB fill between calls, one
event pair per call; median), alternated over `--rounds`; the peak of torch's allocator over one forward + backward; and the largest
difference of the two table gradients.  One JSON line per shape (also appended to `--out`).  Kernel-level times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_win_attn_dtable.py --iters 5 --rounds 1`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

# name, BW, N, heads, dtype, window: stage 1 of config #4 as bench.py --backbone video_swin_t_p4w7 produces it (2 clips x 5 x 384 x 640:
# the window is clamped to (5,7,7)), the same stage with the full window, and the Swin-B stage-1 shape of config #5
SHAPES = [("swin-t stage1 bench (bf16, N=245)", 644, 245, 3, torch.bfloat16, (8, 7, 7)),
          ("swin-t stage1 full window (bf16, N=392)", 270, 392, 3, torch.bfloat16, (8, 7, 7)),
          ("swin-b stage1 (fp16, N=392)", 270, 392, 4, torch.float16, (8, 7, 7))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of a shape's name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ocpg_amd.models.video_swin_transformer as vs
    from ocpg_amd.models.ops.functions.layernorm_func import RelPosBias, StaticGather
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes, window_attention, window_attention_table
    dev = torch.device("cuda:0")
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)          # 1 GiB: four times the Infinity Cache
    for name, bw, n, h, dtype, window in SHAPES:
        if a.only and a.only not in name:
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        idx2 = vs.WindowAttention3D(32 * h, window, h).to(dev).relative_position_index[:n, :n]
        rows = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
        qkv = torch.randn(bw, n, 3, h, 32, device=dev, generator=g).to(dtype).requires_grad_(True)
        table = (torch.randn(rows, h, device=dev, generator=g) * 0.5).requires_grad_(True)
        nw = max(1, bw // 2)
        region = torch.randint(0, 3, (nw, n), device=dev, generator=g).int()
        go = torch.randn(bw, n, h * 32, device=dev, generator=g).to(dtype)
        plan, codes, scale = StaticGather.plan(idx2.reshape(-1), rows), table_codes(idx2), 32 ** -0.5

        def unfused():
            bias, bias_t = RelPosBias.apply(table, idx2, plan)
            return window_attention(qkv, bias, region, scale, nw, bias_t)

        def fused():
            return window_attention_table(qkv, table, idx2, region, scale, nw, codes)

        paths = {"unfused": unfused, "fused": fused}
        rec = {"shape": name, "bw": bw, "n": n, "heads": h, "dtype": str(dtype), "iters": a.iters, "rounds": a.rounds}
        grads, b2b, cold = {}, {k: [] for k in paths}, {k: [] for k in paths}
        for k, fn in paths.items():                       # warm-up, results, allocator peak of one forward + backward
            for _ in range(2):
                torch.autograd.grad(fn(), (qkv, table), go)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            grads[k] = torch.autograd.grad(fn(), (qkv, table), go)
            torch.cuda.synchronize()
            rec[f"{k}_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        for _ in range(a.rounds):
            for k, fn in paths.items():
                out = fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    torch.autograd.grad(out, (qkv, table), go, retain_graph=True)
                e1.record()
                torch.cuda.synchronize()
                b2b[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
                ts = []
                for _ in range(5):
                    flush.fill_(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    torch.autograd.grad(out, (qkv, table), go, retain_graph=True)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                cold[k].append(statistics.median(ts))
        for k in paths:
            rec[f"{k}_bwd_back_to_back_us"] = [round(v, 1) for v in b2b[k]]
            rec[f"{k}_bwd_cold_us"] = [round(v, 1) for v in cold[k]]
        rec["dtable_max_abs_diff"] = (grads["fused"][1] - grads["unfused"][1]).abs().max().item()
        rec["dtable_max_abs"] = grads["unfused"][1].abs().max().item()
        rec["dqkv_equal"] = bool(torch.equal(grads["fused"][0], grads["unfused"][0]))
        rec["lds_adds_per_call"] = bw * h * n * n
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
