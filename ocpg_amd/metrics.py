"""Referring-segmentation metrics of the A2D-Sentences / JHMDB-Sentences evaluation (reference datasets/a2d_eval.py:29-67, fed by
engine.py:158-189): mask IoU, precision@K, overall IoU, mean IoU -- as one batched tensor program on whatever device the masks are on
(the reference decodes COCO RLE annotations one instance at a time on the host; the COCO-style AP numbers it also prints need
pycocotools and are not reproduced here)."""
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
