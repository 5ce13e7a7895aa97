"""A/B of the PNG writers: Pillow on host planes (the default, png="pil") against the run-length encoder on the device
(csrc/png_rle.hip through models/ops/functions/png_func.py, png="native"), on one GPU, in one process, the legs alternated call by
call.  Wall-clock milliseconds per call with the device idle before and after (the calls end in host work: files or bytes).

Inputs: 36 frames each.
  masks_480   binary 0 / 255 planes of 480 x 854, two moving blobs
  masks_720   the same at 720 x 1280
  labels_480  label maps of 3 objects at 480 x 854 with the DAVIS palette

Legs per input:
  encode   the planes are on the device; `pil`: .cpu().numpy() and Image.save into memory per frame; `native`: png_encode
  writer   the whole inference.write_expression_masks(native=True) call (a stand-in model whose forward_selected returns stride-4
           logits made beforehand, one video of 36 JPEG frames in a temporary directory, frames passed through unresized) or
           inference.write_label_maps call into a temporary directory, png="pil" against png="native"
`native_again` is the native leg once more per round: the difference of the two medians is the spread of identical legs.
`native_wins`: rounds in which native beat pil by more than that spread.  File bytes are summed on both sides.  One JSON line per
input in profiles/png_ab.jsonl.

--kernels-only encodes the masks_720 planes a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
for per-kernel times.
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

from ocpg_amd import inference
from ocpg_amd.models.ops.functions.png_func import png_encode

FRAMES = 36
INPUTS = {"masks_480": ("masks", 480, 854), "masks_720": ("masks", 720, 1280), "labels_480": ("labels", 480, 854)}


def blobs(h, w, objects, frames=FRAMES):
    """-> int64 [frames, h, w]: 0 = background, i + 1 inside ellipse i, the ellipses drifting from frame to frame."""
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out = torch.zeros(frames, h, w, dtype=torch.int64)
    for t in range(frames):
        for i in range(objects):
            cy, cx = h * (0.3 + 0.2 * i) + 2 * t, w * (0.25 + 0.22 * i) + 3 * t
            ry, rx = h * (0.18 - 0.03 * i), w * (0.12 + 0.02 * i)
            out[t][((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1] = i + 1
    return out


def timed(fns, iters):
    """Alternate the callables; -> per-callable list of per-call wall-clock milliseconds."""
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
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def compare(pil, native, iters):
    """-> the legs' statistics, the spread of identical legs and the rounds native won by more than it."""
    for _ in range(2):
        pil(), native()
    mp, mn, mn2 = timed([pil, native, native], iters)
    sp, sn, sn2 = stats(mp), stats(mn), stats(mn2)
    spread = abs(sn["median_ms"] - sn2["median_ms"]) / max(min(sn["median_ms"], sn2["median_ms"]), 1e-6)
    return {"pil": sp, "native": sn, "native_again": sn2, "identical_legs_spread": round(spread, 4),
            "native_wins": sum(n * (1 + spread) < p for n, p in zip(mn, mp)), "rounds": iters,
            "pil_over_native": round(sp["median_ms"] / sn["median_ms"], 2)}


def tree_bytes(folder):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(folder) for f in files if f.endswith(".png"))


class StandIn(torch.nn.Module):
    """forward_selected hands back stride-4 logits made beforehand: the writer's own work is all that is timed."""

    def __init__(self, low):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=low.device))
        self.low = low

    def forward_selected(self, clips, captions, targets):
        t = clips[0].shape[0]
        return {"pred_logits": torch.full((1, t, 1, 1), 3.0, device=self.low.device), "pred_masks_low": self.low[None, :t], "mask_up": 4}


def dataset(root, h, w):
    rng = np.random.default_rng(0)
    names = ["%05d" % i for i in range(FRAMES)]
    os.makedirs(os.path.join(root, "valid", "JPEGImages", "vid"))
    os.makedirs(os.path.join(root, "meta_expressions", "valid"))
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for n in names:
        Image.fromarray(frame).save(os.path.join(root, "valid", "JPEGImages", "vid", n + ".jpg"))
    with open(os.path.join(root, "meta_expressions", "valid", "meta_expressions.json"), "w") as f:
        json.dump({"videos": {"vid": {"frames": names, "expressions": {"0": {"exp": "the blobs"}}}}}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_ab.jsonl"))
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_ab.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    if args.kernels_only:
        planes = ((blobs(720, 1280, 2) > 0).to(torch.uint8) * 255).to(dev)
        for _ in range(5):
            png_encode(planes)
        torch.cuda.synchronize()
        return
    lines = []
    for name, (kind, h, w) in INPUTS.items():
        tmp = tempfile.mkdtemp(prefix="png_ab_")
        try:
            if kind == "masks":
                inside = blobs(h, w, 2) > 0
                planes = (inside.to(torch.uint8) * 255).to(dev)
                palette = None
                # stride-4 logits whose x4 replication, cropped, thresholds to blobs of the same kind
                low = torch.where(blobs((h + 3) // 4, (w + 3) // 4, 2) > 0, 8.0, -8.0).to(dev)
                dataset(tmp, h, w)
                model = StandIn(low)

                def same(clip, target):
                    return clip.float(), target

                def writer(png):
                    out = os.path.join(tmp, "out_" + png)
                    n = inference.write_expression_masks(model, tmp, "valid", out, native=True, transform=same, png=png)
                    assert n == FRAMES
                    return out
            else:
                planes = blobs(h, w, 3).to(torch.uint8).to(dev)
                palette = inference.label_palette()

                def writer(png):
                    out = os.path.join(tmp, "out_" + png)
                    inference.write_label_maps(planes, out, palette, png=png)
                    return out

            def encode_pil():
                files = []
                for plane in planes.cpu().numpy():
                    img = Image.fromarray(plane)
                    if palette is not None:
                        img.putpalette(palette)
                    buf = io.BytesIO()
                    img.save(buf, format="PNG")
                    files.append(buf.getvalue())
                return files

            def encode_native():
                return png_encode(planes, palette)
            a, b = encode_pil(), encode_native()
            same_pixels = all(np.array_equal(np.array(Image.open(io.BytesIO(x))), np.array(Image.open(io.BytesIO(y)))) for x, y in zip(a, b))
            d = {"input": name, "frames": FRAMES, "size": [h, w], "encode": compare(encode_pil, encode_native, args.iters),
                 "encode_bytes": {"pil": sum(map(len, a)), "native": sum(map(len, b))},
                 "writer": compare(lambda: writer("pil"), lambda: writer("native"), args.iters)}
            d["writer_bytes"] = {"pil": tree_bytes(writer("pil")), "native": tree_bytes(writer("native"))}
            d["native_over_pil_bytes"] = round(d["writer_bytes"]["native"] / d["writer_bytes"]["pil"], 2)
            d["same_pixels"] = same_pixels
            d["device"] = torch.cuda.get_device_name(0)
            d["host_cpus"] = os.cpu_count()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print(json.dumps(d), flush=True)
        lines.append(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
