"""Referee for the DAVIS-2017 J&F scoring: a literal numpy / scipy restatement of the reference's db_eval_iou, f_measure, _seg2bmap
(davis2017/metrics.py), db_statistics (davis2017/utils.py) and the two _evaluate_* methods (davis2017/evaluation.py), written
independently of the product code, plus the seeded inputs the tests share.

The reference's own module cannot be executed (it needs cv2, skimage and pandas, and uses np.bool).  Stand-ins, by their documented
semantics: scipy.ndimage.binary_dilation(..., border_value=0) for cv2.dilate with its default border (outside pixels never win),
a comparison against r^2 for skimage.morphology.disk, plain bool for np.bool.
"""
import functools
import warnings

import numpy as np
from scipy.ndimage import binary_dilation, gaussian_filter
from scipy.optimize import linear_sum_assignment


# ---- davis2017/metrics.py ---------------------------------------------------------------------------------------------------------
def db_eval_iou(annotation, segmentation, void_pixels=None):
    assert annotation.shape == segmentation.shape
    annotation = annotation.astype(bool)
    segmentation = segmentation.astype(bool)
    if void_pixels is not None:
        assert annotation.shape == void_pixels.shape
        void_pixels = void_pixels.astype(bool)
    else:
        void_pixels = np.zeros_like(segmentation)
    inters = np.sum((segmentation & annotation) & np.logical_not(void_pixels), axis=(-2, -1))
    union = np.sum((segmentation | annotation) & np.logical_not(void_pixels), axis=(-2, -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
    if j.ndim == 0:
        j = 1 if np.isclose(union, 0) else j
    else:
        j[np.isclose(union, 0)] = 1
    return j


def disk(radius):
    """skimage.morphology.disk"""
    a = np.arange(-radius, radius + 1)
    x, y = np.meshgrid(a, a)
    return (x ** 2 + y ** 2 <= radius ** 2).astype(np.uint8)


def seg2bmap(seg):
    """_seg2bmap at width = w, height = h"""
    seg = seg.astype(bool)
    e = np.zeros_like(seg)
    s = np.zeros_like(seg)
    se = np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def bound_pixels(shape, bound_th=0.008):
    return bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape))


def f_measure_parts(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    """f_measure, also returning what it counted: (F, n_fg, n_gt, sum(fg_match), sum(gt_match))"""
    if void_pixels is not None:
        void_pixels = void_pixels.astype(bool)
    else:
        void_pixels = np.zeros_like(foreground_mask).astype(bool)
    bound_pix = int(bound_pixels(foreground_mask.shape, bound_th))
    fg_boundary = seg2bmap(foreground_mask * np.logical_not(void_pixels))
    gt_boundary = seg2bmap(gt_mask * np.logical_not(void_pixels))
    fg_dil = binary_dilation(fg_boundary, structure=disk(bound_pix), border_value=0)
    gt_dil = binary_dilation(gt_boundary, structure=disk(bound_pix), border_value=0)
    gt_match = gt_boundary * fg_dil
    fg_match = fg_boundary * gt_dil
    n_fg = np.sum(fg_boundary)
    n_gt = np.sum(gt_boundary)
    if n_fg == 0 and n_gt > 0:
        precision = 1
        recall = 0
    elif n_fg > 0 and n_gt == 0:
        precision = 0
        recall = 1
    elif n_fg == 0 and n_gt == 0:
        precision = 1
        recall = 1
    else:
        precision = np.sum(fg_match) / float(n_fg)
        recall = np.sum(gt_match) / float(n_gt)
    if precision + recall == 0:
        F = 0
    else:
        F = 2 * precision * recall / (precision + recall)
    return F, int(n_fg), int(n_gt), int(np.sum(fg_match)), int(np.sum(gt_match))


def f_measure(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    return f_measure_parts(foreground_mask, gt_mask, void_pixels, bound_th)[0]


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    assert annotation.shape == segmentation.shape and annotation.ndim == 3
    f_res = np.zeros(annotation.shape[0])
    for frame_id in range(annotation.shape[0]):
        void_pixels_frame = None if void_pixels is None else void_pixels[frame_id]
        f_res[frame_id] = f_measure(segmentation[frame_id], annotation[frame_id], void_pixels_frame, bound_th=bound_th)
    return f_res


# ---- davis2017/utils.py -----------------------------------------------------------------------------------------------------------
def db_statistics(per_frame_values):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        M = np.nanmean(per_frame_values)
        O = np.nanmean(per_frame_values > 0.5)
    N_bins = 4
    ids = np.round(np.linspace(1, len(per_frame_values), N_bins + 1) + 1e-10) - 1
    ids = ids.astype(np.uint8)
    D_bins = [per_frame_values[ids[i]:ids[i + 1] + 1] for i in range(0, 4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        D = np.nanmean(D_bins[0]) - np.nanmean(D_bins[3])
    return M, O, D


# ---- davis2017/evaluation.py, davis.py:get_all_masks, results.py:read_masks ----------------------------------------------------
def evaluate_semisupervised(all_gt_masks, all_res_masks, all_void_masks, bound_th=0.008):
    if all_res_masks.shape[0] > all_gt_masks.shape[0]:
        raise SystemExit("index higher than the number of objects")
    elif all_res_masks.shape[0] < all_gt_masks.shape[0]:
        zero_padding = np.zeros((all_gt_masks.shape[0] - all_res_masks.shape[0], *all_res_masks.shape[1:]))
        all_res_masks = np.concatenate([all_res_masks, zero_padding], axis=0)
    j_metrics_res, f_metrics_res = np.zeros(all_gt_masks.shape[:2]), np.zeros(all_gt_masks.shape[:2])
    for ii in range(all_gt_masks.shape[0]):
        j_metrics_res[ii, :] = db_eval_iou(all_gt_masks[ii, ...], all_res_masks[ii, ...], all_void_masks)
        f_metrics_res[ii, :] = db_eval_boundary(all_gt_masks[ii, ...], all_res_masks[ii, ...], all_void_masks, bound_th)
    return j_metrics_res, f_metrics_res


def evaluate_unsupervised(all_gt_masks, all_res_masks, all_void_masks, max_n_proposals=20, bound_th=0.008):
    if all_res_masks.shape[0] > max_n_proposals:
        raise SystemExit("index higher than the maximum number of proposals")
    elif all_res_masks.shape[0] < all_gt_masks.shape[0]:
        zero_padding = np.zeros((all_gt_masks.shape[0] - all_res_masks.shape[0], *all_res_masks.shape[1:]))
        all_res_masks = np.concatenate([all_res_masks, zero_padding], axis=0)
    j_metrics_res = np.zeros((all_res_masks.shape[0], all_gt_masks.shape[0], all_gt_masks.shape[1]))
    f_metrics_res = np.zeros((all_res_masks.shape[0], all_gt_masks.shape[0], all_gt_masks.shape[1]))
    for ii in range(all_gt_masks.shape[0]):
        for jj in range(all_res_masks.shape[0]):
            j_metrics_res[jj, ii, :] = db_eval_iou(all_gt_masks[ii, ...], all_res_masks[jj, ...], all_void_masks)
            f_metrics_res[jj, ii, :] = db_eval_boundary(all_gt_masks[ii, ...], all_res_masks[jj, ...], all_void_masks, bound_th)
    all_metrics = (np.mean(j_metrics_res, axis=2) + np.mean(f_metrics_res, axis=2)) / 2
    row_ind, col_ind = linear_sum_assignment(-all_metrics)
    return j_metrics_res[row_ind, col_ind, :], f_metrics_res[row_ind, col_ind, :]


def split_gt(masks):
    """DAVIS.get_all_masks(seq, True) on decoded label maps [T, H, W] -> (object masks [G, T, H, W], void [T, H, W])"""
    masks = masks.astype(np.float64)
    masks_void = masks == 255
    masks = np.where(masks_void, 0, masks)
    num_objects = int(np.max(masks[0, ...]))
    ids = np.arange(1, num_objects + 1)[:, None, None, None]
    return (ids == masks[None, ...]), masks_void


def split_res(masks):
    """Results.read_masks on decoded label maps"""
    num_objects = int(np.max(masks))
    ids = np.arange(1, num_objects + 1)[:, None, None, None]
    return ids == masks[None, ...].astype(np.float64)


def evaluate_sequence(gt, res, task, bound_th=0.008):
    """DAVISEvaluation.evaluate's body for one sequence of decoded label maps -> (J, F) [objects, frames]"""
    all_gt_masks, all_void_masks = split_gt(gt)
    if task == "semi-supervised":
        all_gt_masks, res = all_gt_masks[:, 1:-1], res[1:-1]
        return evaluate_semisupervised(all_gt_masks, split_res(res), None, bound_th)
    return evaluate_unsupervised(all_gt_masks, split_res(res), all_void_masks, bound_th=bound_th)


def evaluate_dataset(sequences, task):
    """sequences {name: (gt, res)} -> (the seven global measures in eval_davis.py's order, {'<seq>_<i>': (J mean, F mean)})"""
    J = {"M": [], "R": [], "D": [], "M_per_object": {}}
    F = {"M": [], "R": [], "D": [], "M_per_object": {}}
    for seq, (gt, res) in sequences.items():
        j_res, f_res = evaluate_sequence(gt, res, task)
        for ii in range(j_res.shape[0]):
            for store, values in ((J, j_res[ii]), (F, f_res[ii])):
                m, r, d = db_statistics(values)
                store["M"].append(m)
                store["R"].append(r)
                store["D"].append(d)
                store["M_per_object"][f"{seq}_{ii + 1}"] = m
    final_mean = (np.mean(J["M"]) + np.mean(F["M"])) / 2.
    g_res = [final_mean, np.mean(J["M"]), np.mean(J["R"]), np.mean(J["D"]), np.mean(F["M"]), np.mean(F["R"]), np.mean(F["D"])]
    return g_res, {k: (J["M_per_object"][k], F["M_per_object"][k]) for k in J["M_per_object"]}


# ---- counts: what the kernel returns, from the same pieces ------------------------------------------------------------------------
def reference_counts(gt, res, num_gt, num_res, radius, void_label, all_pairs):
    """-> int32 [P, T, 6]: |A&B|, |A|B|, |b(A)|, |b(B)|, matched b(A), matched b(B); pairs as ocpg_jf_counts_u8 orders them"""
    T = gt.shape[0]
    void = gt == void_label if void_label is not None else np.zeros(gt.shape, dtype=bool)
    pairs = [(r, g) for r in range(num_res) for g in range(num_gt)] if all_pairs else [(g, g) for g in range(num_gt)]
    out = np.zeros((len(pairs), T, 6), dtype=np.int32)
    for p, (r, g) in enumerate(pairs):
        seg, ann = res == r + 1, gt == g + 1
        for t in range(T):
            nv = np.logical_not(void[t])
            out[p, t, 0] = np.sum((seg[t] & ann[t]) & nv)
            out[p, t, 1] = np.sum((seg[t] | ann[t]) & nv)
            out[p, t, 2:] = f_measure_parts(seg[t], ann[t], void[t], bound_th=radius)[1:]
    return out


def jf_from_counts(counts):
    """J and F [P, T] from counts by the reference's branches, scalar by scalar"""
    J, F = np.zeros(counts.shape[:2]), np.zeros(counts.shape[:2])
    for p in range(counts.shape[0]):
        for t in range(counts.shape[1]):
            i, u, n_fg, n_gt, m_fg, m_gt = (int(x) for x in counts[p, t])
            J[p, t] = 1 if u == 0 else i / u
            if n_fg == 0 and n_gt > 0:
                precision, recall = 1, 0
            elif n_fg > 0 and n_gt == 0:
                precision, recall = 0, 1
            elif n_fg == 0 and n_gt == 0:
                precision, recall = 1, 1
            else:
                precision, recall = m_fg / float(n_fg), m_gt / float(n_gt)
            F[p, t] = 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return J, F


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def blobs(seed, T, H, W, num_objects, sigma=None):
    """Smooth-noise label maps [T, H, W] uint8 with ids 0 .. num_objects"""
    rng = np.random.default_rng(seed)
    sigma = max(0.6, min(H, W) / 12.0) if sigma is None else sigma
    out = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        fields = [np.full((H, W), 0.8)]
        for _ in range(num_objects):
            f = gaussian_filter(rng.standard_normal((H, W)), sigma, mode="wrap")
            fields.append(f / (f.std() + 1e-12))
        out[t] = np.argmax(np.stack(fields), axis=0)
    return out


# (T, H, W, radius): the smallest shapes where the kernel can go wrong -- one pixel; narrower than a word; odd sizes under and over one
# 64-column word and one 32-row tile; exact multiples of the tile; one past them; several tiles each way with the largest served
# radius; one native-size clip.  The kernel's tile is 64 x 32, under 100 pixels a side.
SHAPES = [(1, 1, 1, 1), (2, 5, 3, 1), (3, 37, 83, 1), (3, 37, 83, 2), (3, 37, 83, 3), (2, 64, 64, 1), (2, 64, 64, 8), (2, 65, 129, 3),
          (2, 65, 129, 18), (1, 70, 130, 18), (1, 200, 300, 4), (1, 200, 300, 64), (2, 480, 854, 8)]
SPECIAL = ["identical", "empty_result", "empty_gt", "both_empty", "full_frame", "touch_last_row_col", "checkerboard", "corner_pixels",
           "void_stripe"]
SPECIAL_SHAPE = (1, 23, 70, 2)            # crosses a word boundary


def _shape_cases():
    cases = {}
    for i, (T, H, W, r) in enumerate(SHAPES):
        big = H * W > 50000                                # the referee's dilation is slow: fewer pairs at the large shapes
        objects = 1 if big and r > 8 else (2 if big else 1 + i % 3)
        # alternate: result = ground truth rolled by radius + 1, or drawn from another seed; all pairs with R != G on every third
        cases[f"blobs_{T}x{H}x{W}_r{r}"] = dict(kind="roll" if i % 2 == 0 else "seed", T=T, H=H, W=W, radius=r, num_gt=objects,
                                                all_pairs=(i % 3 == 1 and not big), void=(i % 4 == 2), seed=100 + i)
    return cases


CASES = _shape_cases()
for _n in SPECIAL:
    CASES[_n] = dict(kind=_n, T=SPECIAL_SHAPE[0], H=SPECIAL_SHAPE[1], W=SPECIAL_SHAPE[2], radius=SPECIAL_SHAPE[3], num_gt=1,
                     all_pairs=False, void=(_n == "void_stripe"), seed=0)
CASES["corner_pixels"]["num_gt"] = 4
CASES["corner_pixels"]["all_pairs"] = True


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (gt, res uint8 [T, H, W], num_gt, num_res, radius, void_label or None, all_pairs); the arrays are shared: do not write"""
    c = CASES[name]
    T, H, W, r, G, kind = c["T"], c["H"], c["W"], c["radius"], c["num_gt"], c["kind"]
    R = G
    gt = np.zeros((T, H, W), dtype=np.uint8)
    res = np.zeros((T, H, W), dtype=np.uint8)
    if kind in ("roll", "seed"):
        gt = blobs(c["seed"], T, H, W, G)
        if kind == "roll":
            res = np.roll(gt, (r + 1, -(r + 1)), axis=(1, 2))
        else:
            R = G + 1 if c["all_pairs"] else G
            res = blobs(c["seed"] + 1000, T, H, W, R)
        if c["void"]:
            gt = gt.copy()
            gt[:, :, W // 3:W // 3 + max(1, W // 10)] = 255
    elif kind == "identical":
        gt[:, 4:15, 10:68] = 1
        res = gt.copy()
    elif kind == "empty_result":
        gt[:, 4:15, 10:68] = 1
    elif kind == "empty_gt":
        res[:, 4:15, 10:68] = 1
    elif kind == "both_empty":
        pass
    elif kind == "full_frame":                             # no boundary at all: the last row / column / corner rules
        gt[:] = 1
        res[:] = 1
        res[:, :, :3] = 0
    elif kind == "touch_last_row_col":
        gt[:, H - 6:, W - 9:] = 1
        res[:, H - 8:, W - 7:] = 1
    elif kind == "checkerboard":
        yy, xx = np.mgrid[:H, :W]
        gt[:] = ((yy + xx) % 2).astype(np.uint8)
        res[:] = ((yy + xx + 1) % 2).astype(np.uint8) * (xx < W - 5)
    elif kind == "corner_pixels":
        for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            gt[:, y, x] = k + 1
        res = gt.copy()
        res[:, 1, 1] = 1                                     # something for the corner objects to match or miss
        res[:, H - 2, W - 4] = 4
        R = 4
    elif kind == "void_stripe":
        gt[:, 5:18, 20:60] = 1
        res[:, 7:20, 17:57] = 1
        gt[:, :, 38:41] = 255
    else:
        raise KeyError(kind)
    gt.setflags(write=False)
    res.setflags(write=False)
    return gt, res, G, R, r, (255 if c["void"] else None), c["all_pairs"]


@functools.lru_cache(maxsize=None)
def case_counts(name, radius_offset=0, void=True):
    """The referee's counts for a case (computed once per process); void=False scores the same maps with no void label."""
    gt, res, G, R, r, void_label, all_pairs = case_inputs(name)
    out = reference_counts(gt, res, G, R, r + radius_offset, void_label if void else None, all_pairs)
    out.setflags(write=False)
    return out


# ---- a synthetic DAVIS folder -----------------------------------------------------------------------------------------------------
def dataset_sequences(task):
    """{name: (gt, res)} uint8 label maps of three short sequences: permuted proposals with a void stripe; fewer proposals than
    objects; a sequence whose result misses a frame's object (empty masks, every F branch)."""
    H, W = 40, 72
    a = blobs(7, 6, H, W, 3)
    perm = np.array([0, 2, 3, 1], dtype=np.uint8)
    a_res = perm[np.roll(a, (1, 2), axis=(1, 2))]
    b = blobs(8, 5, H, W, 2)
    b_res = np.where(np.roll(b, 2, axis=2) == 1, 1, 0).astype(np.uint8)
    c = blobs(9, 7, H, W, 1)
    c_res = np.roll(c, (2, -1), axis=(1, 2)).copy()
    c_res[2] = 0
    c = c.copy()
    c[4] = 0
    if task == "unsupervised":
        a = a.copy()
        a[:, :, 30:33] = 255
    else:
        a_res = np.roll(a, (1, 2), axis=(1, 2))              # ids must line up in the semi-supervised task
    return {"alpha": (a, a_res), "beta": (b, b_res), "gamma-x": (c, c_res)}


def write_davis_tree(root, task, subset="val", resolution="480p"):
    """Writes dataset_sequences(task) as palette PNGs in the reference's layout -> (davis_root, results_path, sequences)"""
    import os

    from PIL import Image
    seqs = dataset_sequences(task)
    davis, results = os.path.join(root, "davis"), os.path.join(root, "results")
    os.makedirs(os.path.join(davis, "ImageSets", "2017"))
    with open(os.path.join(davis, "ImageSets", "2017", f"{subset}.txt"), "w") as f:
        f.write("\n".join(seqs) + "\n")
    folder = "Annotations" if task == "semi-supervised" else "Annotations_unsupervised"
    palette = np.random.default_rng(0).integers(0, 256, 768).tolist()
    for name, (gt, res) in seqs.items():
        for base, maps in ((os.path.join(davis, folder, resolution, name), gt), (os.path.join(results, name), res)):
            os.makedirs(base)
            for t in range(maps.shape[0]):
                im = Image.fromarray(maps[t], mode="P")
                im.putpalette(palette)
                im.save(os.path.join(base, "%05d.png" % t))
    return davis, results, seqs
