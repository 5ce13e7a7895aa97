"""A/B of the native RoBERTa text encoder (csrc/roberta.hip, models/text_encoder/roberta_native.py) against HF's eager forward, on one
GPU, in one process, the sides alternated call by call.

(a) encoder: RoBERTa-base's shape (12 layers, random init, fp32, eval), B in {1, 2}, L in {8, 20, 40}: wall time per call (host clock
             around the call and a device synchronise, which is what an inference caller waits for) of HF, of the native runner with
             its dense products through ocpg_gemm, and through ocpg_small_linear_f32_fwd; the two halves of every side's samples are
             reported separately (the spread of identical runs), and what the outputs differ by.
(b) gemm:    the four layer shapes at R = 8 .. 80 rows through both entry points: device time per call (events around 20 calls back to
             back), next to the weight-read floor of the shape at 8 TB/s.
(c) infer:   inference.segment_video(native=True) at config #2 (ResNet-101, 4 + 4 layers, bf16 autocast), 36 frames of 480 x 854 in
             clips of 12, one expression: the per-clip encode of the loop as it was before TextEncoder.precompute (restated here: a
             forward_selected call with the string per clip), the encode-once loop with the switch off, and with the switch on.
(d) trace:   `--parts trace --side hf|native`: 10 encoder calls at B = 1, L = 20 and nothing else, for a kernel-trace run of the
             profiler around this tool (launches per call = kernel dispatches / 10, after the 3 warm-up calls it reports).

One JSON line per measurement, appended to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

HBM_GBS = 8000.0
LAYER_SHAPES = (("qkv", 768, 2304), ("attn_out", 768, 768), ("ffn_in", 768, 3072), ("ffn_out", 3072, 768))


def wall(fns, iters):
    """Alternate the callables; -> per-callable list of per-call milliseconds, host clock, each call ended by a synchronise."""
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    half = len(ms) // 2
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "calls": len(ms),
            "median_first_half_ms": round(statistics.median(ms[:half]), 4), "median_second_half_ms": round(statistics.median(ms[half:]), 4)}


def base_model(dev, layers=12):
    from transformers import RobertaConfig, RobertaModel
    torch.manual_seed(0)
    cfg = RobertaConfig(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0,
                        eos_token_id=2, num_hidden_layers=layers)
    model = RobertaModel(cfg).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def tokens(b, l, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 50265, (b, l), generator=g)
    ids[:, 0] = 0
    ids[:, -1] = 2
    if b > 1:
        ids[1, l - l // 4 - 1] = 2
        ids[1, l - l // 4:] = 1
    return ids, ids.ne(1).long()


def encoder_ab(dev, iters, emit):
    from ocpg_amd.models.ops.functions import roberta_func as rf
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward, why_not
    model = base_model(dev)

    def hf(ids, att):
        with torch.no_grad():
            enc = model(input_ids=ids.to(dev), attention_mask=att.to(dev))
        return enc.last_hidden_state, enc.pooler_output

    def native(route, ids, att):
        rf.ROUTE = route
        try:
            return roberta_forward(model, ids, att)
        finally:
            rf.ROUTE = "auto"

    for b in (1, 2):
        for l in (8, 20, 40):
            ids, att = tokens(b, l)
            assert why_not(model, ids) is None
            sides = [("hf", lambda: hf(ids, att)), ("native_gemm", lambda: native("gemm", ids, att)),
                     ("native_small_linear", lambda: native("small", ids, att)), ("native_auto", lambda: native("auto", ids, att))]
            outs = [fn() for _, fn in sides]
            diff = {name + "_vs_hf_max_abs": round(max((o[0] - outs[0][0]).abs().max().item(), (o[1] - outs[0][1]).abs().max().item()), 9)
                    for (name, _), o in zip(sides[1:], outs[1:])}
            for _, fn in sides:
                for _ in range(3):
                    fn()
            ms = wall([fn for _, fn in sides], iters)
            emit({"part": "encoder", "B": b, "L": l, "layers": 12, "small_rows": rf.SMALL_ROWS,
                  **{name: stats(m) for (name, _), m in zip(sides, ms)}, **diff})


def gemm_ab(dev, iters, emit):
    from ocpg_amd.models.ops.functions import roberta_func as rf
    g = torch.Generator().manual_seed(1)
    reps = 20
    for name, k, n in LAYER_SHAPES:
        w = (torch.randn(n, k, generator=g) * 0.05).to(dev)
        bias = torch.randn(n, generator=g).to(dev)
        floor_us = 4.0 * n * k / (HBM_GBS * 1e3)
        for r in (8, 16, 20, 40, 64, 80):
            x = torch.randn(r, k, generator=g).to(dev)
            fns = [lambda: rf.linear(x, w, bias, route="small"), lambda: rf.linear(x, w, bias, route="gemm")]
            diff = (fns[0]() - fns[1]()).abs().max().item()
            us = [[], []]
            for fn in fns:
                for _ in range(5):
                    fn()
            for _ in range(iters):
                for i, fn in enumerate(fns):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[i].append(e0.elapsed_time(e1) * 1e3 / reps)
            emit({"part": "gemm", "shape": name, "R": r, "K": k, "N": n, "small_linear_us": round(statistics.median(us[0]), 2),
                  "ocpg_gemm_us": round(statistics.median(us[1]), 2), "small_linear_min_us": round(min(us[0]), 2),
                  "ocpg_gemm_min_us": round(min(us[1]), 2), "weight_read_floor_us": round(floor_us, 2), "max_abs_diff": diff,
                  "note": "device events around 20 back-to-back calls: includes the launch rate of the stream"})


def infer_ab(dev, iters, emit):
    import bench
    from ocpg_amd import inference
    from ocpg_amd.models import build_model
    from ocpg_amd.models.ops.functions.mask_tail_func import mask_probabilities
    frames_n, h, w, clip = 36, 480, 854, 12
    torch.manual_seed(0)
    args = bench.model_args(dev, "resnet101", amp=True, roberta=True)
    args.dataset_file = "davis"
    model, _, _ = build_model(args)
    model.to(dev).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    frames = torch.randn(frames_n, 3, h, w, device=dev)
    text = "the person on the left riding a red bike near the tree"
    size = torch.as_tensor([h, w], device=dev)

    def per_clip(native):
        model.text_encoder.native = native
        low = []
        with torch.no_grad():
            for s in range(0, frames_n, clip):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    o = model.forward_selected([frames[s:s + clip]], [text], [{"size": size}])
                low.append(o["pred_masks_low"][0].float())
            return mask_probabilities(torch.cat(low, 0), o["mask_up"], (h, w), (h, w))

    def once(native):
        model.text_encoder.native = native
        return inference.segment_video(model, frames, text, clip_len=clip, amp_dtype=torch.bfloat16, native=True)[1]

    sides = [("per_clip_encode_hf", lambda: per_clip(False)), ("encode_once_hf", lambda: once(False)), ("encode_once_native", lambda: once(True))]
    for _, fn in sides:
        for _ in range(2):
            fn()
    outs = [fn() for _, fn in sides]
    same = {"encode_once_hf_equals_per_clip": bool(torch.equal(outs[0], outs[1])),
            "native_vs_hf_masks_max_abs": (outs[2] - outs[1]).abs().max().item()}
    del outs
    ms = wall([fn for _, fn in sides], iters)
    enc = wall([lambda: model.text_encoder.precompute([text], dev)], iters)            # the switch is on (left by the last side)
    model.text_encoder.native = False
    enc_hf = wall([lambda: model.text_encoder.precompute([text], dev)], iters)
    emit({"part": "infer", "frames": frames_n, "size": [h, w], "clip_len": clip, "expression_words": len(text.split()),
          "model": "config #2 (resnet101, 4+4 layers, 5 queries), initial weights, bf16 autocast, RoBERTa-base random init",
          **{name: stats(m) for (name, _), m in zip(sides, ms)}, "encode_native_alone": stats(enc[0]), "encode_hf_alone_under_no_autocast": stats(enc_hf[0]),
          **same})


def trace(dev, side):
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward
    model = base_model(dev)
    ids, att = tokens(1, 20)
    for i in range(13):
        if side == "native":
            roberta_forward(model, ids, att)
        else:
            with torch.no_grad():
                model(input_ids=ids.to(dev), attention_mask=att.to(dev))
        torch.cuda.synchronize()
    print(json.dumps({"part": "trace", "side": side, "calls": 13, "warmup_calls": 3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_native_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--infer-iters", type=int, default=20)
    ap.add_argument("--parts", default="encoder,gemm,infer")
    ap.add_argument("--side", default="native", choices=("hf", "native"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_native_ab: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    if "trace" in parts:
        return trace(dev, a.side)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if "gemm" in parts:
            gemm_ab(dev, a.iters, emit)
        if "encoder" in parts:
            encoder_ab(dev, a.iters, emit)
        if "infer" in parts:
            infer_ab(dev, a.infer_iters, emit)


if __name__ == "__main__":
    main()
