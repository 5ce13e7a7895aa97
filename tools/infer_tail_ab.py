"""A/B of the native inference tail (csrc/mask_tail.hip, OCPG.forward_selected) against the path it stands in for, on one GPU, in one
process, the two sides alternated call by call, each call between its own pair of device events.

(a) tail:    the ATen chain of inference.py (nearest x4, un-pad crop, bilinear resize, sigmoid [, threshold -> 0 / 255 bytes | stack,
             merge_objects]) against ocpg_mask_tail_f32 modes 0 / 1 / 2.  36 frames, 480 x 864 padded (stride-4 source 120 x 216), crop
             480 x 854, H0 x W0 in {480 x 854, 720 x 1280}, K in {1, 3} objects; source operands warm (re-read straight after the
             previous call) and cold (a buffer larger than L2 + MALL is rewritten before every timed call, outside the events).
(b) forward: OCPG.forward against OCPG.forward_selected in eval on one 36-frame 480 x 854 clip, the config-#2 model (ResNet-101, 4 + 4
             layers, 5 queries, bf16 autocast) from its initial weights; the two results are compared bit for bit.
(c) dynmask: ocpg_dynmask_fwd_f32 at (b)'s shapes: 36 x 20 sets, 36 x 1 sets, and 36 x 1 sets without the pre1 store.

One JSON line per measurement: median / min of the per-call times, the algorithmic bytes of each side (the byte model of DESIGN.md
section 4.8p, computed here from the shapes) and what the outputs differ by.  A time is a device-event interval around everything a
call enqueues, so the chain's many launches and their gaps count, as they do for a user.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import bench
from ocpg_amd import _lib, inference
from ocpg_amd.models.ops.functions import mask_tail_func as M

T, HP, WP, H, W, UP = 36, 480, 864, 480, 854, 4


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "calls": len(ms)}


def old_probabilities(low, origin):
    x = F.interpolate(low[None], scale_factor=UP)                    # the model's eval branch (ocpg.py)
    x = x[:, :, :H, :W]
    return F.interpolate(x, size=origin, mode="bilinear", align_corners=False).sigmoid()[0]


def tail_ab(dev, iters, emit):
    hs, ws = HP // UP, WP // UP
    g = torch.Generator().manual_seed(0)
    coarse = torch.randn(3 * T, 1, hs // 8, ws // 8, generator=g)
    src = (F.interpolate(coarse, size=(hs, ws), mode="bicubic", align_corners=False)[:, 0] * 6
           + 0.5 * torch.randn(3 * T, hs, ws, generator=g)).view(3, T, hs, ws).to(dev)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)       # 1 GiB: past the 256 MB MALL

    def cold():
        flush.add_(1)

    for origin in ((480, 854), (720, 1280)):
        for k in (1, 3):
            s = src[:k].contiguous()
            px = T * origin[0] * origin[1]
            old_model = k * T * (8 * HP * WP + 19 * origin[0] * origin[1])
            sides = {
                "mode0": (lambda: [old_probabilities(s[i], origin) for i in range(k)],
                          lambda: [M.mask_probabilities(s[i], UP, (H, W), origin) for i in range(k)], k * (4 * px + 4 * T * hs * ws)),
                "mode1": (lambda: [(old_probabilities(s[i], origin) > 0.5).to(torch.uint8).mul(255) for i in range(k)],
                          lambda: [M.mask_binary(s[i], UP, (H, W), origin, 0.5, 255) for i in range(k)], k * (px + 4 * T * hs * ws)),
                "mode2": (lambda: inference.merge_objects(torch.stack([old_probabilities(s[i], origin) for i in range(k)])),
                          lambda: M.mask_labels(s, UP, (H, W), origin, 0.3, 0.1), px + k * 4 * T * hs * ws),
            }
            for mode, (old, new, new_model) in sides.items():
                a, b = old(), new()
                if mode == "mode2":
                    diff = {"label_mismatch_share": (a != b).float().mean().item()}
                elif mode == "mode1":
                    diff = {"byte_mismatch_share": max((x != y).float().mean().item() for x, y in zip(a, b))}
                else:
                    diff = {"max_abs_diff": max((x - y).abs().max().item() for x, y in zip(a, b))}
                del a, b
                for _ in range(3):
                    old(), new()
                for state, before in (("warm", None), ("cold", cold)):
                    mo, mn = timed([old, new], iters, before)
                    so, sn = stats(mo), stats(mn)
                    emit({"part": "tail", "mode": mode, "K": k, "frames": T, "src": [hs, ws], "up": UP, "crop": [H, W], "out": list(origin),
                          "operands": state, "aten_chain": so, "mask_tail": sn, "speedup_median": round(so["median_ms"] / sn["median_ms"], 2),
                          "model_bytes_aten_chain": old_model, "model_bytes_mask_tail": new_model,
                          "mask_tail_model_gbs": round(new_model / sn["median_ms"] / 1e6, 1), **diff})


def forward_ab(dev, iters, emit):
    from ocpg_amd.models import build_model
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
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

    def run(selected):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return (model.forward_selected if selected else model)([frames], text, targets)

    for _ in range(2):
        full, sel = run(False), run(True)
    up = F.interpolate(sel["pred_masks_low"].float(), scale_factor=4)[:, :, None]
    same = {"pred_masks_equal": bool(torch.equal(up, full["pred_masks"].float())),
            "pred_masks_max_abs_diff": (up - full["pred_masks"].float()).abs().max().item(),
            "pred_logits_equal": bool(torch.equal(sel["pred_logits"], full["pred_logits"]))}
    del full, sel, up
    mf, ms = timed([lambda: run(False), lambda: run(True)], iters)
    sf, ss = stats(mf), stats(ms)
    emit({"part": "forward", "frames": T, "size": [H, W], "model": "config #2 (resnet101, 4+4 layers, 5 queries), initial weights, bf16 autocast",
          "forward": sf, "forward_selected": ss, "speedup_median": round(sf["median_ms"] / ss["median_ms"], 3), **same})
    # the mask head's own launches inside the two forwards
    for name, selected in (("forward", False), ("forward_selected", True)):
        _lib.enable_kernel_timing(True)
        run(selected)
        kt = _lib.collect_kernel_timing()
        emit({"part": "forward_kernels", "path": name,
              "kernels_ms": {k: {"ms": round(v["ms"], 4), "n": v["n"]} for k, v in kt.items() if k.startswith(("ocpg_dynmask", "ocpg_mso"))}})


def dynmask_ab(dev, iters, emit):
    c, h, w, ch = 256, HP // 8, WP // 8, 16
    npar = (c + 2) * ch + ch * ch + 2 * ch
    feats = torch.randn(T, c, h, w, device=dev)
    L = _lib.lib()

    def make(q, keep):
        params = torch.randn(T * q, npar, device=dev) * 0.05
        ref = torch.rand(T * q, 2, device=dev) * 400
        out = torch.empty(T * q, ch, h, w, device=dev)
        pre1 = torch.empty_like(out) if keep else None

        def fn():
            _lib.check(L.ocpg_dynmask_fwd_f32(feats.data_ptr(), params.data_ptr(), ref.data_ptr(), T, q, c, h, w, 8, out.data_ptr(),
                                              None if pre1 is None else pre1.data_ptr(), _lib.stream_ptr()), "ocpg_dynmask_fwd_f32")
        return fn

    fns = [make(20, True), make(1, True), make(1, False)]
    for fn in fns:
        for _ in range(3):
            fn()
    res = timed(fns, iters)
    emit({"part": "dynmask", "frames": T, "feats": [c, h, w], "sets_720_with_pre1": stats(res[0]), "sets_36_with_pre1": stats(res[1]),
          "sets_36_without_pre1": stats(res[2])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_tail_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--forward-iters", type=int, default=6)
    ap.add_argument("--parts", default="tail,dynmask,forward")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_tail_ab: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        parts = a.parts.split(",")
        if "tail" in parts:
            tail_ab(dev, a.iters, emit)
        if "dynmask" in parts:
            dynmask_ab(dev, a.iters, emit)
        if "forward" in parts:
            forward_ab(dev, a.forward_iters, emit)


if __name__ == "__main__":
    main()
