"""Referring-segmentation metrics of the A2D-Sentences / JHMDB-Sentences evaluation (reference datasets/a2d_eval.py:29-67, fed by
engine.py:158-189): mask IoU, precision@K, overall IoU, mean IoU -- as one batched tensor program on whatever device the masks are on
(the reference decodes COCO RLE annotations one instance at a time on the host; the COCO-style AP numbers it also prints need
pycocotools and are not reproduced here).  The same evaluation from integer counts, with the AP numbers restated from COCOeval's
algorithm, is further down: coco_ap_single_gt, RefMaskAccumulator, load_coco_gt."""
import math
import warnings
from typing import Dict, Sequence

import numpy as np
import torch
from torch import Tensor

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


def mask_iou(pred: Tensor, gt: Tensor, eps: float = 1e-6):
    """pred, gt [N, H, W] (bool / 0-1) -> (iou [N], intersection [N], union [N]); (I + eps) / (U + eps): two empty masks count as
    IoU 1 -- a2d_eval.py:29-34."""
    p, g = pred.bool(), gt.bool()
    inter = (p & g).flatten(1).sum(1).to(torch.float32)
    union = (p | g).flatten(1).sum(1).to(torch.float32)
    return (inter + eps) / (union + eps), inter, union


def select_best_query(scores: Tensor, masks: Tensor) -> Tensor:
    """scores [N, Q], masks [N, Q, H, W] -> the mask of the highest-scoring query per instance [N, H, W] (a2d_eval.py:47-48: the
    prediction with the highest score; on equal scores the reference's stable sort keeps the LAST one, as here)."""
    q = scores.shape[1]
    best = q - 1 - scores.flip(1).argmax(dim=1)
    return masks[torch.arange(masks.shape[0], device=masks.device), best]


def precision_and_iou(pred: Tensor, gt: Tensor, thresholds: Sequence[float] = THRESHOLDS) -> Dict[str, float]:
    """One prediction and one ground-truth mask per instance ([N, H, W] each) -> {'P@0.5'..'P@0.9', 'overall_iou', 'mean_iou'}:
    precision@K = share of instances with IoU strictly above K, overall IoU = total intersection / total union, mean IoU = mean of
    the per-instance IoUs -- a2d_eval.py:37-67.  Instances of different sizes: call `accumulate` per batch and `summarize` once."""
    return summarize(accumulate(None, pred, gt), thresholds)


def accumulate(state, pred: Tensor, gt: Tensor):
    """Adds a batch to the running sums (state = None to start): (ious list, total intersection, total union)."""
    iou, inter, union = mask_iou(pred, gt)
    if state is None:
        return [iou], inter.sum(), union.sum()
    return state[0] + [iou], state[1] + inter.sum(), state[2] + union.sum()


def summarize(state, thresholds: Sequence[float] = THRESHOLDS) -> Dict[str, float]:
    ious = torch.cat(state[0])
    out = {"P@%s" % k: float((ious > k).float().mean()) for k in thresholds}
    out["overall_iou"] = float(state[1] / state[2]) if float(state[2]) > 0 else 0.0      # all masks empty: no union
    out["mean_iou"] = float(ious.mean())
    return out


# ---- DAVIS-2017 J&F (reference eval_davis.py, davis2017/evaluation.py, metrics.py, utils.py) -------------------------------------
# The pixel work is six integer counts per (pair, frame) (models/ops/functions/jf_func.py: one HIP kernel on the GPU); everything
# below is the reference's fp64 host arithmetic on those counts.  Not reproduced: the temporal metric (the reference refuses it too)
# and the averaging over Ref-DAVIS's four annotators (the caller loops).

VOID_LABEL = 255
MAX_PROPOSALS = 20
GLOBAL_MEASURES = ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")


def boundary_radius(h: int, w: int, bound_th: float = 0.008) -> int:
    """The disk radius of f_measure (metrics.py:77-78): bound_th >= 1 is taken as pixels, otherwise ceil(bound_th * |(h, w)|_2) in
    fp64 -- 8 at 480 x 854, 18 at 1080 x 1920."""
    if bound_th >= 1:
        return int(bound_th)
    return int(math.ceil(bound_th * math.sqrt(float(h * h + w * w))))


def jf_from_counts(counts: Tensor):
    """counts [P, T, 6] integers (jf_counts) -> (J, F), fp64 [P, T] on the CPU, with the reference's branches:
    J = I / U, and 1 where U = 0 (db_eval_iou);  precision = matched b(A) / |b(A)|, recall = matched b(B) / |b(B)| with
    (|b(A)|, |b(B)|) = (0, >0): (1, 0), (>0, 0): (0, 1), (0, 0): (1, 1);  F = 2 P R / (P + R), and 0 where P + R = 0 (f_measure)."""
    c = counts.detach().to("cpu", torch.float64)
    inter, union, n_res, n_gt, m_res, m_gt = c.unbind(-1)
    one, zero = torch.ones_like(inter), torch.zeros_like(inter)
    j = torch.where(union == 0, one, inter / union.clamp(min=1))
    precision = torch.where(n_res == 0, one, torch.where(n_gt == 0, zero, m_res / n_res.clamp(min=1)))
    recall = torch.where(n_gt == 0, one, torch.where(n_res == 0, zero, m_gt / n_gt.clamp(min=1)))
    s = precision + recall
    f = torch.where(s == 0, zero, 2 * precision * recall / torch.where(s == 0, one, s))
    return j, f


def db_statistics(values):
    """Per-frame values of one object -> (mean, recall, decay) (utils.py:135-161): nanmean; the share of frames > 0.5 (a NaN frame
    counts as a miss); the mean of the first quarter minus the mean of the last, over the reference's four bins ids = round(linspace(1,
    n, 5) + 1e-10) - 1, closed on both ends.  The bin ends are plain integers here: the reference casts them to uint8, which wraps
    past 256 frames and then slices the wrong frames -- no DAVIS sequence is that long."""
    v = np.asarray(values, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mean = float(np.nanmean(v))
        recall = float(np.nanmean(v > 0.5))
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
        decay = float(np.nanmean(v[ids[0]:ids[1] + 1]) - np.nanmean(v[ids[3]:ids[4] + 1]))
    return mean, recall, decay


def davis_sequence_jf(gt: Tensor, res: Tensor, task: str = "unsupervised", bound_th: float = 0.008, native=None):
    """One sequence: gt, res uint8 label maps [T, H, W] on any device -> (J, F), fp64 [objects, frames] on the CPU.

    'unsupervised' (the reference's default; evaluation.py:44-64): pixels with gt == 255 are void, the objects are 1 .. max of frame
    0 without void, the proposals 1 .. max of res (more than 20 raises; fewer than objects are padded with empty ones), every
    (proposal, object) pair is scored and scipy's linear_sum_assignment on -(mean J + mean F) / 2 picks one proposal per object.
    As in the reference the rows come out in the order of the chosen PROPOSALS, not of the objects.
    'semi-supervised' (evaluation.py:28-41, 85): no void (255 is background), first and last frame dropped, result id k scored
    against object k, missing ids as empty masks, more result ids than objects raises."""
    from scipy.optimize import linear_sum_assignment

    from .models.ops.functions.jf_func import jf_counts
    if gt.dim() != 3 or gt.shape != res.shape:
        raise ValueError(f"davis_sequence_jf: expected two [T, H, W] label maps, got {tuple(gt.shape)} and {tuple(res.shape)}")
    if task not in ("unsupervised", "semi-supervised"):
        raise ValueError("davis_sequence_jf: task is 'unsupervised' or 'semi-supervised'")
    first = gt[0]
    num_gt = int(torch.where(first == VOID_LABEL, torch.zeros_like(first), first).max())
    radius = boundary_radius(gt.shape[1], gt.shape[2], bound_th)
    if task == "semi-supervised":
        gt, res = gt[1:-1], res[1:-1]
        if gt.shape[0] == 0:
            raise ValueError("davis_sequence_jf: the semi-supervised task needs more than two frames")
    frames = gt.shape[0]
    num_res = int(res.max())
    empty = torch.zeros((0, frames), dtype=torch.float64)
    if task == "semi-supervised":
        if num_res > num_gt:
            raise ValueError("davis_sequence_jf: the results hold an index higher than the number of objects in the sequence")
        if num_gt == 0:
            return empty, empty
        return jf_from_counts(jf_counts(gt, res, num_gt, radius=radius, native=native))
    if num_res > MAX_PROPOSALS:
        raise ValueError(f"davis_sequence_jf: the results hold an index higher than the {MAX_PROPOSALS} proposals allowed")
    if num_gt == 0:
        return empty, empty
    num_res = max(num_res, num_gt)
    j, f = jf_from_counts(jf_counts(gt, res, num_gt, num_res, radius=radius, void_label=VOID_LABEL, all_pairs=True, native=native))
    j, f = j.reshape(num_res, num_gt, frames), f.reshape(num_res, num_gt, frames)
    score = (np.mean(j.numpy(), axis=2) + np.mean(f.numpy(), axis=2)) / 2
    rows, cols = linear_sum_assignment(-score)
    return j[rows, cols], f[rows, cols]


class DavisAccumulator:
    """Collects the per-object statistics of eval_davis.py: add(seq, J, F) per sequence, then summary()."""

    def __init__(self):
        self.stats = {"J": {"M": [], "R": [], "D": []}, "F": {"M": [], "R": [], "D": []}}
        self.per_object = {}                                  # '<seq>_<i>' -> (J mean, F mean), in insertion order

    def add(self, seq: str, j, f):
        for i in range(len(j)):
            means = []
            for key, values in (("J", j[i]), ("F", f[i])):
                m, r, d = db_statistics(values)
                for k, x in zip("MRD", (m, r, d)):
                    self.stats[key][k].append(x)
                means.append(m)
            self.per_object[f"{seq}_{i + 1}"] = tuple(means)

    def summary(self):
        """-> ({measure: value} for GLOBAL_MEASURES, {'<seq>_<i>': (J mean, F mean)})."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            g = {f"{k}-{name}": float(np.mean(self.stats[k][s])) for k in "JF" for s, name in zip("MRD", ("Mean", "Recall", "Decay"))}
        g["J&F-Mean"] = (g["J-Mean"] + g["F-Mean"]) / 2.0
        return {k: g[k] for k in GLOBAL_MEASURES}, dict(self.per_object)


# ---- A2D-Sentences / JHMDB-Sentences from counts (reference engine.py:158-189, datasets/a2d_eval.py, pycocotools' COCOeval) -------------
# Every figure of this evaluation is a function of three integers per (sample, query) -- |P & G|, |P|, |G|
# (models/ops/functions/refmask_func.py: one HIP kernel per batch on the GPU) -- and the query's score: the task has one ground-truth
# mask per image, no crowd regions, and categories are ignored.  Everything below is host arithmetic on those integers.

AP_LABELS = ("mAP 0.5:0.95", "AP 0.5", "AP 0.75", "AP 0.5:0.95 S", "AP 0.5:0.95 M", "AP 0.5:0.95 L")
COCO_IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
COCO_RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
COCO_MAX_DETS = 100
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large


def _np(x, dtype):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dtype)


def coco_ap_single_gt(scores, counts, gt_area=None, order=None) -> Dict[str, float]:
    """scores [N, Q], counts [N, Q, 3] = (|P & G|, |P|, |G|) per image and detection -> the reference's six AP figures (AP_LABELS).

    Restates pycocotools' COCOeval (evaluate + accumulate + summarize) with iouType='segm', useCats=0 for ONE non-crowd ground truth
    per image, in fp64 numpy, vectorised over images, detections and IoU thresholds: IoU = I / (|P| + |G| - I) and 0 where the union
    is 0; thresholds linspace(.5, .95, 10); recall points linspace(0, 1, 101); maxDets 100; area ranges all / small / medium / large.
    Per image and range the ground truth is ignored when gt_area (default |G|; the reference's JSON carries an `area` field) lies
    outside the range; detections go by descending score (stable: ties keep query order); the first whose IoU reaches
    min(t, 1 - 1e-10) takes the ground truth and inherits its ignore flag; an unmatched detection whose own area |P| lies outside
    the range is ignored.  All detections are then merged by a stable descending sort on score -- images in `order` (a permutation of
    range(N): ascending image_id; default insertion order) -- ignored ones are dropped, cumulative TP / FP give recall = TP / (ground
    truths not ignored) and precision = TP / (TP + FP + spacing(1)), precision is made non-increasing from the right and sampled at
    the first index with recall >= r for each recall point (0 past the end).  AP = mean over thresholds and recall points, -1 where a
    range has no ground truth that is not ignored.
    Not reproduced: COCOeval tests `dtm == 0` for "unmatched", which confuses a ground truth whose annotation id is 0 with no match;
    here a match is a match whatever the id."""
    s = _np(scores, np.float64)
    c = _np(counts, np.int64)
    if s.ndim != 2 or c.shape != s.shape + (3,):
        raise ValueError(f"coco_ap_single_gt: expected scores [N, Q] and counts [N, Q, 3], got {s.shape} and {c.shape}")
    n = s.shape[0]
    if order is not None:
        order = np.asarray(order, dtype=np.int64)
        s, c = s[order], c[order]
    area = c[:, 0, 2].astype(np.float64) if gt_area is None else _np(gt_area, np.float64)[order if order is not None else slice(None)]
    if n == 0:
        return {k: -1.0 for k in AP_LABELS}
    rank = np.argsort(-s, axis=1, kind="stable")[:, :COCO_MAX_DETS]
    s = np.take_along_axis(s, rank, 1)
    inter = np.take_along_axis(c[..., 0], rank, 1).astype(np.float64)
    det_area = np.take_along_axis(c[..., 1], rank, 1).astype(np.float64)
    union = det_area + c[:, :1, 2] - inter
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)
    thr = np.minimum(COCO_IOU_THRESHOLDS, 1 - 1e-10)
    reach = iou[None] >= thr[:, None, None]                                      # [T, N, D]
    match = reach & (np.cumsum(reach, axis=2) == 1)                              # the first that reaches it takes the one ground truth
    flat_order = np.argsort(-s.reshape(-1), kind="stable")                       # merged over images
    match_f = match.reshape(len(thr), -1)[:, flat_order]
    ap = np.full((len(COCO_AREA_RANGES), len(thr)), -1.0)
    for a, (lo, hi) in enumerate(COCO_AREA_RANGES):
        gt_ignored = (area < lo) | (area > hi)                                   # [N]
        n_gt = int((~gt_ignored).sum())
        if n_gt == 0:
            continue
        det_out = (det_area < lo) | (det_area > hi)                              # [N, D]
        ignored = np.where(match, gt_ignored[None, :, None], det_out[None])      # [T, N, D]
        ignored_f = ignored.reshape(len(thr), -1)[:, flat_order]
        for t in range(len(thr)):
            tp = match_f[t][~ignored_f[t]]
            ctp = np.cumsum(tp, dtype=np.float64)
            cfp = np.cumsum(~tp, dtype=np.float64)
            recall = ctp / n_gt
            precision = ctp / (ctp + cfp + np.spacing(1))
            precision = np.maximum.accumulate(precision[::-1])[::-1]
            at = np.searchsorted(recall, COCO_RECALL_THRESHOLDS, side="left")
            ap[a, t] = np.append(precision, 0.0)[at].mean()                       # at == len(precision): past the end, 0

    def mean(x):
        x = x[x > -1]
        return float(x.mean()) if x.size else -1.0
    t50, t75 = int(np.argmin(np.abs(COCO_IOU_THRESHOLDS - 0.5))), int(np.argmin(np.abs(COCO_IOU_THRESHOLDS - 0.75)))
    values = (mean(ap[0]), mean(ap[0, t50:t50 + 1]), mean(ap[0, t75:t75 + 1]), mean(ap[1]), mean(ap[2]), mean(ap[3]))
    return dict(zip(AP_LABELS, values))


class RefMaskAccumulator:
    """Collects scores and counts of the A2D / JHMDB evaluation: add(...) per batch, gather() with a process group, summary() once.

    summary() returns the 13 keys of reference engine.py:183-189: the six AP figures (coco_ap_single_gt, images in ascending image_id
    order as COCOeval sorts them) and P@0.5 .. P@0.9, overall_iou, mean_iou of the highest-scoring query per image (on equal scores
    the last one, as select_best_query), with the per-instance IoU (I + 1e-6) / (U + 1e-6) in fp32 as mask_iou, their mean in fp64 and
    the overall sums in int64 -- exact, as the reference's Python floats are.  An image_id added more than once (a sampler that pads
    the last batch) counts once, the first time."""

    def __init__(self):
        self.image_ids, self.scores, self.counts, self.areas = [], [], [], []

    def add(self, image_ids, scores, counts, gt_area=None):
        """image_ids: B hashable, sortable ids; scores [B, Q]; counts [B, Q, 3]; gt_area: B numbers or None (|G|)."""
        s, c = _np(scores, np.float32), _np(counts, np.int64)
        if s.ndim != 2 or c.shape != s.shape + (3,) or len(image_ids) != s.shape[0]:
            raise ValueError(f"RefMaskAccumulator.add: expected B ids, scores [B, Q], counts [B, Q, 3]; got {len(image_ids)}, {s.shape}, {c.shape}")
        area = c[:, 0, 2].astype(np.float64) if gt_area is None else _np(gt_area, np.float64).reshape(-1)
        for i, image_id in enumerate(image_ids):
            self.image_ids.append(image_id.item() if torch.is_tensor(image_id) else image_id)
            self.scores.append(s[i])
            self.counts.append(c[i])
            self.areas.append(float(area[i]))

    def gather(self):
        """With a process group: every rank ends with all ranks' samples, in rank order (a few bytes per sample; the reference gathers
        every run-length string).  Every rank must call it, also one that added nothing."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, (self.image_ids, self.scores, self.counts, self.areas))
        self.image_ids, self.scores, self.counts, self.areas = ([x for p in parts for x in p[k]] for k in range(4))
        return self

    def summary(self, thresholds: Sequence[float] = THRESHOLDS) -> Dict[str, float]:
        seen, keep = set(), []
        for i, image_id in enumerate(self.image_ids):
            if image_id not in seen:
                seen.add(image_id)
                keep.append(i)
        if not keep:
            return {}
        if len({len(self.scores[i]) for i in keep}) != 1:
            raise ValueError("RefMaskAccumulator: the number of queries changed between batches")
        scores = np.stack([self.scores[i] for i in keep])
        counts = np.stack([self.counts[i] for i in keep])
        areas = np.asarray([self.areas[i] for i in keep])
        ids = [self.image_ids[i] for i in keep]
        out = coco_ap_single_gt(scores, counts, areas, order=sorted(range(len(ids)), key=lambda i: ids[i]))
        q = scores.shape[1]
        best = q - 1 - np.argmax(scores[:, ::-1], axis=1)
        c = counts[np.arange(len(ids)), best]
        inter, union = c[:, 0], c[:, 1] + c[:, 2] - c[:, 0]
        eps = np.float32(1e-6)
        ious = (inter.astype(np.float32) + eps) / (union.astype(np.float32) + eps)
        out.update({"P@%s" % k: float((ious > np.float32(k)).mean()) for k in thresholds})
        total_union = int(union.sum())
        out["overall_iou"] = int(inter.sum()) / total_union if total_union > 0 else 0.0
        out["mean_iou"] = float(ious.astype(np.float64).mean())
        return out


def load_coco_gt(path) -> Dict:
    """The reference's `*_annotations_in_coco_format.json` (engine.py:171-174) -> {image_id: (mask uint8 tensor [H0, W0], area)}: one
    annotation per image, its `segmentation` a COCO run-length encoding read by models/postprocessors.py:rle_decode; `area` is the
    JSON's field, or the mask's own where it is missing."""
    import json

    from .models.postprocessors import rle_decode
    with open(path) as f:
        data = json.load(f)
    out = {}
    for ann in data["annotations"]:
        if ann["image_id"] in out:
            raise ValueError(f"load_coco_gt: more than one annotation for image {ann['image_id']!r}")
        if ann.get("iscrowd", 0):
            raise ValueError(f"load_coco_gt: crowd annotation on image {ann['image_id']!r}")
        mask = rle_decode(ann["segmentation"])
        out[ann["image_id"]] = (torch.from_numpy(mask), float(ann["area"]) if "area" in ann else float(mask.sum()))
    return out


def write_coco_results(path, samples):
    """samples: [(image_id, [score per query], [run-length dict per query])] of this rank -> the reference's prediction list
    (engine.py:158-163) as JSON at `path`, written by rank 0 after a gather over the ranks, in rank order.  Every rank must call it,
    also one without samples.  Returns the list on rank 0, None elsewhere."""
    import json

    import torch.distributed as dist
    preds = []
    for image_id, scores, rles in samples:
        for s, m in zip(scores, rles):
            counts = m["counts"]
            preds.append({"image_id": image_id, "category_id": 1,                    # a dummy label, as the reference has it
                          "segmentation": {"size": [int(v) for v in m["size"]], "counts": counts.decode("ascii") if isinstance(counts, bytes) else counts},
                          "score": float(s)})
    rank = 0
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, preds)
        preds, rank = [p for part in parts for p in part], dist.get_rank()
    if rank != 0:
        return None
    with open(path, "w") as f:
        json.dump(preds, f)
    return preds


def load_coco_results(path) -> Dict:
    """A prediction list as write_coco_results makes it -> {image_id: [(score, mask uint8 tensor [H0, W0])]}, the queries of an image
    in the file's order; an image_id that JSON turned into a list comes back as a tuple."""
    import json

    from .models.postprocessors import rle_decode
    with open(path) as f:
        data = json.load(f)
    out = {}
    for p in data:
        image_id = tuple(p["image_id"]) if isinstance(p["image_id"], list) else p["image_id"]
        out.setdefault(image_id, []).append((float(p["score"]), torch.from_numpy(rle_decode(p["segmentation"]))))
    return out
