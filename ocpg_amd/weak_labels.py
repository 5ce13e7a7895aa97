"""Weak annotations from frames and masks: the per-frame point / box similarity heat maps the method trains from (reference
pre_process/generate_anno_ytvos.py:50-105, pre_process/sim_model.py:14-141).

    mask  ->  centre point + box            mask_centers_and_boxes   (exact integers, any device)
    frame ->  ResNet features               SimilarityLabeler        (the package's own ResNetBody)
    features + point / box -> heat maps     ops/functions/sim_heat_func.sim_heat (csrc/sim_heat.hip or its torch composition)
    dataset tree -> AnnotationsWeakly/      write_weak_annotations, `python -m ocpg_amd.weak_labels`

The files written (`<frame>.npz` with obj_ids, heatBBox, heatPoint, centerPoint) are the ones datasets/video_folders.py:
default_weak_loader reads.  The dense-CRF refinement (pre_process/dense_crf.py) is not part of this: neither generate script calls it.
"""
import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .models.ops.functions.sim_heat_func import MAX_CANDIDATES, sim_heat

# OpenCV's 5x5 chamfer weights for DIST_L2 at 16 fractional bits: a = 1 (axial), b = 1.4 (diagonal), c = 2.1969 (knight move)
CHAMFER_A, CHAMFER_B, CHAMFER_C = 65536, 91750, 143976
_FAR = 1 << 40              # "no source seen yet": above every real distance, far below the int64 range

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def chamfer_distance_5x5(masks: Tensor) -> Tensor:
    """masks [N, H, W] (non-zero = object) -> int64 [N, H, W]: the two-pass 5x5 chamfer distance to the nearest zero pixel in 1/65536
    pixel units; 0 on the zero pixels; pixels outside the frame are never sources.  A mask without a zero pixel has no finite distance
    (values >= 2^40).

    The sequential recurrence inside a row, t[j] = min(c[j], t[j-1] + a), equals a*j + cummin(c[k] - a*k), so each pass is one batched
    step per row over all N masks, exact in int64."""
    fg = masks != 0
    n, h, w = fg.shape
    dev = fg.device
    a, b, c = CHAMFER_A, CHAMFER_B, CHAMFER_C
    t = torch.full((n, h + 4, w + 4), _FAR, dtype=torch.int64, device=dev)          # frame of 2: outside never wins
    ramp = a * torch.arange(w, dtype=torch.int64, device=dev)

    def sweep(v):
        return torch.cummin(v - ramp, dim=1).values + ramp

    def from_rows(r1, r2):
        """r1 the adjacent row, r2 the one beyond it (both with the frame): the best of the 7 neighbours they hold."""
        m = torch.minimum(r2[:, 1:w + 1], r2[:, 3:w + 3]) + c
        m = torch.minimum(m, torch.minimum(r1[:, 0:w], r1[:, 4:w + 4]) + c)
        m = torch.minimum(m, torch.minimum(r1[:, 1:w + 1], r1[:, 3:w + 3]) + b)
        return torch.minimum(m, r1[:, 2:w + 2] + a)

    zero = torch.zeros((), dtype=torch.int64, device=dev)
    for i in range(h):                                                                # forward: rows above, then left to right
        v = torch.where(fg[:, i], from_rows(t[:, i + 1], t[:, i]), zero)
        t[:, i + 2, 2:w + 2] = sweep(v)
    for i in range(h - 1, -1, -1):                                                    # backward: rows below, then right to left
        v = torch.minimum(t[:, i + 2, 2:w + 2], from_rows(t[:, i + 3], t[:, i + 4]))
        t[:, i + 2, 2:w + 2] = sweep(v.flip(1)).flip(1)
    return t[:, 2:h + 2, 2:w + 2].contiguous()


def mask_centers_and_boxes(masks: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """bool / 0-1 masks [N, H, W] on any device -> (centers int64 [N, 2] as (x, y), boxes int64 [N, 4] as (x1, y1, x2, y2), valid int64 [N]).

    Centre (generate_anno_ytvos.py:73-76): the first maximum, in raster order, of the 5x5 chamfer distance transform, taken over the
    integer fixed-point distances.  The reference calls cv2.distanceTransform(mask, DIST_L2, 5); OpenCV is not a dependency here, so
    parity with it rests on OpenCV's documented algorithm (two raster passes over the 5x5 neighbourhood with the fixed-point weights
    65536 / 91750 / 143976, pixels outside the frame never sources), restated in chamfer_distance_5x5 -- as the dilation of
    ops/functions/jf_func.py rests on cv2.dilate's.  A mask with no zero pixel has no defined centre (OpenCV's values saturate):
    ValueError.
    Box: the reference's bounding_box -- first and last occupied column and row, the last one inclusive.
    An empty mask gives valid 0, centre (0, 0) and box (0, 0, 0, 0) (generate_anno_ytvos.py:87-90)."""
    if masks.dim() != 3:
        raise ValueError(f"mask_centers_and_boxes: expected [N, H, W], got {tuple(masks.shape)}")
    fg = masks != 0
    n, h, w = fg.shape
    dev = fg.device
    if n == 0:
        z = torch.zeros((0,), dtype=torch.int64, device=dev)
        return z.view(0, 2), z.view(0, 4), z
    if min(h, w) < 1:
        raise ValueError("mask_centers_and_boxes: empty frame")
    if bool(fg.flatten(1).all(1).any()):
        raise ValueError("mask_centers_and_boxes: a mask without a background pixel has no distance transform")
    valid = fg.flatten(1).any(1)
    dist = chamfer_distance_5x5(fg).flatten(1)
    cells = torch.arange(h * w, dtype=torch.int64, device=dev)[None]
    first = torch.where(dist == dist.amax(1, keepdim=True), cells, h * w).amin(1)
    centers = torch.stack([first % w, first // w], dim=1)
    cols, rows = fg.any(1), fg.any(2)                                                 # [N, W], [N, H]
    xs = torch.arange(w, dtype=torch.int64, device=dev)[None]
    ys = torch.arange(h, dtype=torch.int64, device=dev)[None]
    boxes = torch.stack([torch.where(cols, xs, w).amin(1), torch.where(rows, ys, h).amin(1),
                         torch.where(cols, xs, -1).amax(1), torch.where(rows, ys, -1).amax(1)], dim=1)
    keep = valid[:, None]
    return centers * keep, boxes * keep, valid.to(torch.int64)


def point_cell(center: Sequence[float], frame_hw: Tuple[int, int], map_hw: Tuple[int, int]) -> Tuple[int, int]:
    """Frame pixel (x, y) -> feature cell (x, y), in Python floats and the reference's order of operations (sim_model.py:45-48 on the
    normalised point of generate_anno_ytvos.py:77)."""
    (fh, fw), (h, w) = frame_hw, map_hw
    return int(float(center[0]) / fw * w), int(float(center[1]) / fh * h)


def box_candidates(box: Sequence[float], frame_hw: Tuple[int, int], map_hw: Tuple[int, int]) -> Tuple[List[int], List[Tuple[int, int]]]:
    """Frame box (x1, y1, x2, y2) -> (the box in feature cells, the candidate cells) as sim_model.py:80-98: the scaled ends truncated,
    every cell of the inclusive ranges, the stride grown by 1 until at most 256 remain, x outer and y inner."""
    (fh, fw), (h, w) = frame_hw, map_hw
    cur = [int(float(box[0]) / fw * w), int(float(box[1]) / fh * h), int(float(box[2]) / fw * w), int(float(box[3]) / fh * h)]
    xs, ys = list(range(cur[0], cur[2] + 1)), list(range(cur[1], cur[3] + 1))
    i = 1
    while len(xs) * len(ys) > MAX_CANDIDATES:
        xs, ys = list(range(cur[0], cur[2] + 1, i + 1)), list(range(cur[1], cur[3] + 1, i + 1))
        i += 1
    return cur, [(x, y) for x in xs for y in ys]


class SimilarityLabeler(nn.Module):
    """The reference's SimModel on this package's kernels: a ResNet body (parameter names are torchvision's, so a DenseCL checkpoint's
    ["state_dict"] loads with strict=False, sim_model.py:30-33) and the similarity head on its last stage.  Always in eval mode under
    no_grad.  `native` is passed to sim_heat (None: its default path)."""

    def __init__(self, backbone: str = "resnet101", dilation: bool = False, checkpoint: Optional[str] = None, frames_per_pass: int = 4,
                 native: Optional[bool] = None):
        super().__init__()
        from .models.backbone import ResNetBody
        self.body = ResNetBody(backbone, dilation, return_interm_layers=False)
        self.frames_per_pass, self.native = int(frames_per_pass), native
        if checkpoint is not None:
            state = torch.load(checkpoint, map_location="cpu")
            self.body.load_state_dict(state["state_dict"] if "state_dict" in state else state, strict=False)
        self.eval()

    def train(self, mode: bool = True):
        return super().train(False)

    @torch.no_grad()
    def features(self, frames: Tensor) -> Tensor:
        """ImageNet-normalised frames [F, 3, H, W] -> fp32 [F, h, w, C], channels contiguous per pixel."""
        out = []
        for i in range(0, frames.shape[0], self.frames_per_pass):
            x = frames[i:i + self.frames_per_pass]
            if x.is_cuda:                                      # the body's own kernels serve channels-last maps
                x = x.contiguous(memory_format=torch.channels_last)
            y = self.body(x)["0"]
            out.append(y.permute(0, 2, 3, 1).to(torch.float32).contiguous())
        return torch.cat(out)

    @torch.no_grad()
    def label_frames(self, frames: Tensor, centers: Tensor, boxes: Tensor, valid: Tensor) -> Tuple[Tensor, Tensor]:
        """frames [F, 3, H, W] (ImageNet-normalised, full resolution), centers [F, n, 2] (x, y), boxes [F, n, 4] (x1, y1, x2, y2, the
        last column / row inclusive), valid [F, n] -> (heat_point, heat_box), both fp32 [F, n, h, w]; an object that is not valid gets
        zero planes (sim_model.py:62-63,131-132).  The candidate lists are built on the host; per chunk of frames_per_pass frames the
        head is one sim_heat call per mode."""
        nf, _, fh, fw = frames.shape
        n = centers.shape[1]
        centers, boxes, valid = centers.tolist(), boxes.tolist(), valid.tolist()
        points, planes = [], []
        for i in range(0, nf, self.frames_per_pass):
            feat = self.features(frames[i:i + self.frames_per_pass])
            k, h, w, _ = feat.shape
            obj_frame = torch.arange(k).repeat_interleave(n)
            p_off, p_xy, b_off, b_xy, b_box = [0], [], [0], [], []
            for f in range(i, i + k):
                for o in range(n):
                    cells, cur = [], [0, 0, 0, 0]
                    if valid[f][o]:
                        p_xy.append(point_cell(centers[f][o], (fh, fw), (h, w)))
                        cur, cells = box_candidates(boxes[f][o], (fh, fw), (h, w))
                    p_off.append(len(p_xy))
                    b_xy += cells
                    b_off.append(len(b_xy))
                    b_box.append(cur)
            as_xy = lambda v: torch.tensor(v, dtype=torch.int32).view(-1, 2)
            hp = sim_heat(feat, obj_frame, torch.tensor(p_off), as_xy(p_xy), None, native=self.native)[0]
            hb = sim_heat(feat, obj_frame, torch.tensor(b_off), as_xy(b_xy), torch.tensor(b_box, dtype=torch.int32).view(-1, 4),
                          native=self.native)[0]
            points.append(hp.view(k, n, h, w))
            planes.append(hb.view(k, n, h, w))
        return torch.cat(points), torch.cat(planes)


def objects_by_frame(root: str, split: str):
    """videos -> (object ids named by the expressions, in order of first mention; every listed frame) -- the reference's
    transform_anno_to_each_frame (generate_anno_ytvos.py:30-48)."""
    with open(os.path.join(root, "meta_expressions", split, "meta_expressions.json")) as f:
        videos = json.load(f)["videos"]
    out = {}
    for vid, v in videos.items():
        ids = []
        for e in v["expressions"].values():
            if int(e["obj_id"]) not in ids:
                ids.append(int(e["obj_id"]))
        out[vid] = (ids, list(v["frames"]))
    return out


def _save(path: str, fmt: str, obj_ids, heat_box, heat_point, centers):
    arrays = {"obj_ids": np.asarray(obj_ids, dtype=np.int64), "heatBBox": heat_box, "heatPoint": heat_point,
              "centerPoint": np.asarray(centers, dtype=np.int64).reshape(-1, 2)}
    tmp = path + ".part"                                       # a run that is interrupted leaves no half-written annotation behind
    if fmt == "h5":
        import h5py
        with h5py.File(tmp, "w") as f:
            for k, v in arrays.items():
                f.create_dataset(k, data=v)
    else:
        with open(tmp, "wb") as f:
            np.savez(f, **arrays)
    os.replace(tmp, path)


@torch.no_grad()
def write_weak_annotations(root: str, split: str, labeler: SimilarityLabeler, out_dir: Optional[str] = None, device="cpu",
                           format: str = "npz") -> int:
    """Walk <root>/<split>/{JPEGImages,Annotations} for the objects the expressions name and every listed frame
    (generate_anno_ytvos.py:30-105) and write <out_dir>/<video>/<frame>.npz (default out_dir: <root>/<split>/AnnotationsWeakly, where
    RefVideoClips looks) with obj_ids [n], heatBBox [n, h, w], heatPoint [n, h, w], centerPoint [n, 2].  format "h5" writes the
    reference's files instead and needs h5py.  Frames already written are skipped.  -> the number of files written."""
    from PIL import Image
    if format not in ("npz", "h5"):
        raise ValueError(f"write_weak_annotations: unknown format {format!r}")
    if format == "h5":
        import h5py                                            # noqa: F401  (fail before any work when it is not installed)
    folder = os.path.join(root, split)
    out_dir = out_dir or os.path.join(folder, "AnnotationsWeakly")
    device = torch.device(device)
    labeler = labeler.to(device)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    written = 0
    for vid, (obj_ids, frames) in objects_by_frame(root, split).items():
        os.makedirs(os.path.join(out_dir, vid), exist_ok=True)
        todo = [n for n in frames if not os.path.exists(os.path.join(out_dir, vid, f"{n}.{format}"))]
        for i in range(0, len(todo), labeler.frames_per_pass):
            names = todo[i:i + labeler.frames_per_pass]
            imgs = [np.asarray(Image.open(os.path.join(folder, "JPEGImages", vid, n + ".jpg")).convert("RGB")) for n in names]
            labs = [np.asarray(Image.open(os.path.join(folder, "Annotations", vid, n + ".png")).convert("P")) for n in names]
            if len({x.shape for x in imgs}) > 1:               # frames of one video share a size; if not, one frame per pass
                groups = [[j] for j in range(len(names))]
            else:
                groups = [list(range(len(names)))]
            for g in groups:
                x = torch.from_numpy(np.stack([imgs[j] for j in g])).to(device).permute(0, 3, 1, 2).to(torch.float32) / 255.0
                x = (x - mean) / std
                lab = torch.from_numpy(np.stack([labs[j] for j in g])).to(device)
                ids = torch.tensor(obj_ids, device=device, dtype=lab.dtype).view(1, -1, 1, 1)
                masks = lab[:, None] == ids                                            # [k, n, H, W]
                k, n = masks.shape[:2]
                centers, boxes, valid = mask_centers_and_boxes(masks.flatten(0, 1))
                centers, boxes, valid = centers.view(k, n, 2).cpu(), boxes.view(k, n, 4).cpu(), valid.view(k, n).cpu()
                hp, hb = labeler.label_frames(x, centers, boxes, valid)
                hp, hb = hp.cpu().numpy(), hb.cpu().numpy()
                for r, j in enumerate(g):
                    _save(os.path.join(out_dir, vid, f"{names[j]}.{format}"), format, obj_ids, hb[r], hp[r], centers[r].numpy())
                    written += 1
    return written


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Generate the AnnotationsWeakly heat maps of a Ref-YouTube-VOS / Ref-DAVIS split")
    ap.add_argument("--root", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--checkpoint", default=None, help="DenseCL / torchvision ResNet weights (a state dict or {'state_dict': ...})")
    ap.add_argument("--backbone", default="resnet101", choices=("resnet50", "resnet101"))
    ap.add_argument("--dilation", action="store_true")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--format", default="npz", choices=("npz", "h5"))
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--frames-per-pass", type=int, default=4)
    args = ap.parse_args(argv)
    labeler = SimilarityLabeler(args.backbone, args.dilation, args.checkpoint, args.frames_per_pass)
    n = write_weak_annotations(args.root, args.split, labeler, args.out_dir, args.device, args.format)
    print(json.dumps({"written": n, "root": args.root, "split": args.split}))


if __name__ == "__main__":
    main()
