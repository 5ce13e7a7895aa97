"""Referee of ocpg_amd.metrics.coco_ap_single_gt: the COCOeval algorithm (evaluateImg, accumulate, summarize; iouType 'segm',
useCats 0, one non-crowd ground truth per image) as plain Python loops -- per area range, per image, per threshold, per detection --
on lists and floats.  Nothing is vectorised and ignored detections are kept in the merged list, as COCOeval keeps them (they add to
neither the true nor the false positives), where the product drops them; the two must agree to rounding.
As in the product, a detection is "unmatched" when it took no ground truth: COCOeval's own test `dtm == 0` also fires for a matched
ground truth whose annotation id is 0, which neither side reproduces."""
import numpy as np

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10).tolist()                    # COCOeval's Params: the values themselves, not 0.5 + 0.05 i
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101).tolist()
AREA_RANGES = [(0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)]
MAX_DETS = 100
LABELS = ["mAP 0.5:0.95", "AP 0.5", "AP 0.75", "AP 0.5:0.95 S", "AP 0.5:0.95 M", "AP 0.5:0.95 L"]


def _stable_descending(keys):
    """Indices by descending key, equal keys in their original order (merge sort on the negated key, as COCOeval)."""
    return sorted(range(len(keys)), key=lambda i: -keys[i])             # Python's sort is stable


def evaluate_image(scores, counts, gt_area, lo, hi):
    """One image, one area range -> (sorted scores, matched[t][d], ignored[t][d], ground truth ignored)."""
    gt_ignored = gt_area < lo or gt_area > hi
    order = _stable_descending(list(scores))[:MAX_DETS]
    ious = []
    for d in order:
        inter, pred, g = (int(v) for v in counts[d])
        union = pred + g - inter
        ious.append(inter / union if union > 0 else 0.0)
    matched, ignored = [], []
    for t in IOU_THRESHOLDS:
        taken = False
        m_row, i_row = [], []
        for k, d in enumerate(order):
            need = min(t, 1 - 1e-10)
            hit = (not taken) and not (ious[k] < need)
            if hit:
                taken = True
            m_row.append(hit)
            i_row.append(gt_ignored if hit else False)
        for k, d in enumerate(order):
            area = int(counts[d][1])
            if not m_row[k] and (area < lo or area > hi):
                i_row[k] = True
        matched.append(m_row)
        ignored.append(i_row)
    return [float(scores[d]) for d in order], matched, ignored, gt_ignored


def coco_ap(scores, counts, gt_area=None, order=None):
    n = len(scores)
    images = list(range(n)) if order is None else [int(i) for i in order]
    precision = {}                                                       # (area range, threshold) -> 101 samples, absent = -1
    for a, (lo, hi) in enumerate(AREA_RANGES):
        per_image = []
        for i in images:
            area = float(counts[i][0][2]) if gt_area is None else float(gt_area[i])
            per_image.append(evaluate_image(scores[i], counts[i], area, lo, hi))
        all_scores = [s for e in per_image for s in e[0]]
        merged = _stable_descending(all_scores)
        n_gt = sum(0 if e[3] else 1 for e in per_image)
        if n_gt == 0:
            continue
        for t in range(len(IOU_THRESHOLDS)):
            m = [x for e in per_image for x in e[1][t]]
            ig = [x for e in per_image for x in e[2][t]]
            tp = fp = 0
            rc, pr = [], []
            for j in merged:
                if m[j] and not ig[j]:
                    tp += 1
                if not m[j] and not ig[j]:
                    fp += 1
                rc.append(tp / n_gt)
                pr.append(tp / (fp + tp + np.spacing(1)))
            for j in range(len(pr) - 1, 0, -1):
                if pr[j] > pr[j - 1]:
                    pr[j - 1] = pr[j]
            q = []
            for r in RECALL_THRESHOLDS:
                at = 0
                while at < len(rc) and rc[at] < r:
                    at += 1
                q.append(pr[at] if at < len(pr) else 0.0)
            precision[(a, t)] = q

    def summarize(a, ts):
        vals = [v for t in ts if (a, t) in precision for v in precision[(a, t)]]
        return sum(vals) / len(vals) if vals else -1.0
    every = list(range(len(IOU_THRESHOLDS)))
    stats = [summarize(0, every), summarize(0, [0]), summarize(0, [5]), summarize(1, every), summarize(2, every), summarize(3, every)]
    return dict(zip(LABELS, stats))
