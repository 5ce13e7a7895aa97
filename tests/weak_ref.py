"""Referee of the weak-annotation generator (ocpg_amd/weak_labels.py, ops/functions/sim_heat_func.py, csrc/sim_heat.hip), written from
the definitions and not from the product's code:

  * the 5x5 chamfer distance transform as the plain sequential two-pass in Python integers, first-maximum centre, inclusive box;
  * the similarity head in fp64 with per-candidate scores, the choice and the planes, plus the fp32 error bounds the tests use;
  * the candidate-list construction.
"""
import numpy as np

A, B, C = 65536, 91750, 143976           # 1, 1.4, 2.1969 at 16 fractional bits
FAR = 1 << 40
EPS32 = 2.0 ** -24                       # unit round-off of fp32


# ---------------------------------------------------------------- centres and boxes ----
def chamfer_5x5(mask):
    """mask [H, W] (non-zero = object) -> list of lists of Python ints: distance to the nearest zero pixel, 1/65536 pixel units."""
    h, w = len(mask), len(mask[0])
    t = [[FAR] * (w + 4) for _ in range(h + 4)]          # a frame of 2 that never is a source
    for i in range(h):
        r0, r1, r2 = t[i + 2], t[i + 1], t[i]
        for j in range(w):
            if not mask[i][j]:
                r0[j + 2] = 0
                continue
            r0[j + 2] = min(r2[j + 1] + C, r2[j + 3] + C, r1[j] + C, r1[j + 1] + B, r1[j + 2] + A, r1[j + 3] + B, r1[j + 4] + C,
                            r0[j + 1] + A)
    for i in range(h - 1, -1, -1):
        r0, r1, r2 = t[i + 2], t[i + 3], t[i + 4]
        for j in range(w - 1, -1, -1):
            r0[j + 2] = min(r0[j + 2], r2[j + 3] + C, r2[j + 1] + C, r1[j + 4] + C, r1[j + 3] + B, r1[j + 2] + A, r1[j + 1] + B,
                            r1[j] + C, r0[j + 3] + A)
    return [row[2:w + 2] for row in t[2:h + 2]]


def center_and_box(mask):
    """mask [H, W] -> ((x, y), (x1, y1, x2, y2), valid): first maximum of the transform in raster order; first / last occupied column
    and row (inclusive); an empty mask: (0, 0), (0, 0, 0, 0), 0; a mask without a zero pixel: ValueError."""
    mask = np.asarray(mask) != 0
    if not mask.any():
        return (0, 0), (0, 0, 0, 0), 0
    if mask.all():
        raise ValueError("no background pixel")
    d = chamfer_5x5(mask.tolist())
    best, at = -1, (0, 0)
    for y, row in enumerate(d):
        for x, v in enumerate(row):
            if v > best:
                best, at = v, (x, y)
    ys, xs = np.where(mask.any(1))[0], np.where(mask.any(0))[0]
    return at, (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])), 1


# ---------------------------------------------------------------- candidate lists ----
def point_cell(center, frame_hw, map_hw):
    (fh, fw), (h, w) = frame_hw, map_hw
    return int(center[0] / fw * w), int(center[1] / fh * h)


def box_candidates(box, frame_hw, map_hw):
    """-> (box in cells [x0, y0, x1, y1], candidates [(x, y)]): every cell of the inclusive ranges, stride + 1 until <= 256 remain,
    x outer, y inner."""
    (fh, fw), (h, w) = frame_hw, map_hw
    x0, y0, x1, y1 = int(box[0] / fw * w), int(box[1] / fh * h), int(box[2] / fw * w), int(box[3] / fh * h)
    step = 1
    while True:
        xs, ys = range(x0, x1 + 1, step), range(y0, y1 + 1, step)
        if len(xs) * len(ys) <= 256:
            break
        step += 1
    return [x0, y0, x1, y1], [(x, y) for x in xs for y in ys]


# ---------------------------------------------------------------- similarity head ----
def sim_head(feat, obj_frame, cand_off, cand_xy, box=None):
    """feat [F, h, w, C] -> dict of fp64 results and fp32 error bounds, per candidate (flat index over all objects):

      s [total, h*w]      the rescaled similarity rows            s_bound [total, h*w]   elementwise bound on an fp32 result
      score [total]       box score (0 in point mode)             score_bound [total]
      choice [n_obj]      best candidate per object, lowest index among equals, -1 without candidates

    Bounds, to first order in the unit round-off u = 2^-24 (eps32 = 2^-23 = 2u), times 1.01 for the higher-order terms (the largest
    relative perturbation below is (C + 4) eps32 < 3e-4 at C = 2048):
      a = q^ . k^ :   a C-term fp32 dot product in any order is off by at most C u sum_i |q_i k_i|; each of the two norms is the
                      square root of such a sum of squares (relative C u / 2 + 2u with the reciprocal), applied with one rounding
                      each.  On positive or mixed-sign data alike |a| <= sum_i |q^_i k^_i|, so
                      |da| <= (C + 4) eps32 sum_i |q^_i k^_i|  =: e
      s = (a - mn) / mx :  the fp32 minimum / maximum may sit on another pixel than the exact one, but its value is off by at most the
                      largest e of the row, e_row.  Two roundings (difference, quotient):
                      |ds| <= (e + e_row) / mx + |s| (e_row / mx + 2u)
      mx[x], my[y]:   the bound of a maximum is the largest bound among the elements it ranges over
      num = sum m b, den = sum (m + b - m b) + 1e-5 over n terms, b in {0, 1} so m b is exact and a term with b = 1 is exactly 1:
                      |d num| <= sum b dm + (n + 2) u sum |m b|,   |d den| <= sum (1 - b) dm + (n + 2) u sum (|m| + b + |m b|) + 1e-5 u
      score = (num_x / den_x + num_y / den_y) / 2:  |d(num/den)| <= d_num / den + |num| d_den / den^2 + u |num / den|.
    """
    feat = np.asarray(feat, dtype=np.float64)
    f, h, w, c = feat.shape
    p = h * w
    k = feat.reshape(f, p, c)
    k = k / np.linalg.norm(k, axis=-1, keepdims=True)
    n_obj = len(obj_frame)
    total = int(cand_off[-1])
    s = np.zeros((total, p))
    s_bound = np.zeros((total, p))
    score = np.zeros(total)
    score_bound = np.zeros(total)
    choice = np.full(n_obj, -1, dtype=np.int64)
    u = EPS32
    for o in range(n_obj):
        fr = int(obj_frame[o])
        for ci in range(int(cand_off[o]), int(cand_off[o + 1])):
            x, y = int(cand_xy[ci][0]), int(cand_xy[ci][1])
            q = k[fr, y * w + x]
            a = k[fr] @ q
            e = (c + 4) * 2 * u * (np.abs(k[fr]) @ np.abs(q))
            mn, mx = a.min(), a.max()
            s[ci] = (a - mn) / mx
            em = e.max()
            s_bound[ci] = 1.01 * ((e + em) / mx + np.abs(s[ci]) * (em / mx + 2 * u))
            if box is not None:
                x0, y0, x1, y1 = (int(v) for v in box[o])
                plane, pb = s[ci].reshape(h, w), s_bound[ci].reshape(h, w)
                parts = []
                for m, mb, b in ((plane.max(0), pb.max(0), ((np.arange(w) >= x0) & (np.arange(w) < x1)).astype(np.float64)),
                                 (plane.max(1), pb.max(1), ((np.arange(h) >= y0) & (np.arange(h) < y1)).astype(np.float64))):
                    n = len(m)
                    num, den = (m * b).sum(), (m + b - m * b).sum() + 1e-5
                    d_num = (mb * b).sum() + (n + 2) * u * np.abs(m * b).sum()
                    d_den = (mb * (1 - b)).sum() + (n + 2) * u * (np.abs(m) + b + np.abs(m * b)).sum() + 1e-5 * u
                    parts.append((num / den, 1.01 * (d_num / den + abs(num) * d_den / den ** 2 + u * abs(num / den))))
                score[ci] = 0.5 * (parts[0][0] + parts[1][0])
                score_bound[ci] = 0.5 * (parts[0][1] + parts[1][1]) + u * abs(score[ci])
        lo, hi = int(cand_off[o]), int(cand_off[o + 1])
        if hi > lo:
            choice[o] = int(np.argmax(score[lo:hi]))                      # numpy: the first maximum
    return {"s": s, "s_bound": s_bound, "score": score, "score_bound": score_bound, "choice": choice}


def top2_gap(score, cand_off, o):
    """Gap between the best and the second-best fp64 score of object o (inf with fewer than 2 candidates)."""
    v = np.sort(score[int(cand_off[o]):int(cand_off[o + 1])])
    return float("inf") if len(v) < 2 else float(v[-1] - v[-2])


def positive_features(seed, f, h, w, c):
    """|N(0,1)| + 0.05: no zero vector, every similarity positive."""
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((f, h, w, c))) + 0.05).astype(np.float32)


# ---------------------------------------------------------------- shared fixtures of the head tests ----
def _cells(g, h, w, n):
    """n distinct cells in a seeded order, as (x, y)."""
    return [(int(p % w), int(p // w)) for p in g.choice(h * w, size=n, replace=False)]


def _case(seed, h, w, c, objects, frames=1, point=False):
    """objects: per object (frame, candidate count or explicit cells, box or None = a seeded inner box)."""
    g = np.random.default_rng(seed)
    feat = positive_features(seed, frames, h, w, c)
    obj_frame, off, xy, boxes = [], [0], [], []
    for fr, cand, box in objects:
        cells = _cells(g, h, w, cand) if isinstance(cand, int) else list(cand)
        if box is None:
            x0, y0 = int(g.integers(0, max(1, w // 2))), int(g.integers(0, max(1, h // 2)))
            box = [x0, y0, int(g.integers(x0 + 1, w + 1)), int(g.integers(y0 + 1, h + 1))]
        obj_frame.append(fr), xy.extend(cells), off.append(len(xy)), boxes.append(list(box))
    return {"feat": feat, "obj_frame": np.array(obj_frame, dtype=np.int32), "cand_off": np.array(off, dtype=np.int32),
            "cand_xy": np.array(xy, dtype=np.int32).reshape(-1, 2), "box": None if point else np.array(boxes, dtype=np.int32)}


# name -> (seed, h, w, C, objects, frames, point mode).  The seeds were chosen on the fp64 referee alone so that every object with at
# least two candidates and a non-degenerate box has a top-2 score gap above twice its score bound (asserted by the tests).
HEAD_CASES = {
    "1x1x4_one": (0, 1, 1, 4, [(0, 1, [0, 0, 1, 1])], 1, False),
    "2x3x8_two": (0, 2, 3, 8, [(0, 2, None)], 1, False),
    "3x5x68_corners": (0, 3, 5, 68, [(0, [(0, 0), (4, 0), (0, 2), (4, 2)], None)], 1, False),
    "7x9x2048_17": (0, 7, 9, 2048, [(0, 17, None)], 1, False),
    "23x40x256_multi": (0, 23, 40, 256, [(0, 256, None), (0, 0, None), (1, 17, None), (1, 2, None)], 2, False),
    "45x80x64_256": (0, 45, 80, 64, [(0, 256, None)], 1, False),
    "7x9x8_degenerate_box": (0, 7, 9, 8, [(0, 17, [3, 2, 3, 2])], 1, False),
    "7x9x8_whole_map_box": (0, 7, 9, 8, [(0, 17, [0, 0, 9, 7])], 1, False),
    "7x9x12_point": (0, 7, 9, 12, [(0, 1, None), (1, 0, None), (1, 1, None)], 2, True),
}
DEGENERATE = ("7x9x8_degenerate_box",)

_cache = {}


def head_case(name):
    """-> (inputs dict, referee dict), computed once per process and shared by the tests (treat as read-only)."""
    if name not in _cache:
        seed, h, w, c, objects, frames, point = HEAD_CASES[name]
        case = _case(seed, h, w, c, objects, frames, point)
        _cache[name] = (case, sim_head(case["feat"], case["obj_frame"], case["cand_off"], case["cand_xy"], case["box"]))
    return _cache[name]


def assert_fixture_gap(name):
    """The fixture condition: the referee's own top-2 gap exceeds twice the score bound, so the chosen index is decided."""
    case, ref = head_case(name)
    if case["box"] is None or name in DEGENERATE:
        return
    off = case["cand_off"]
    for o in range(len(case["obj_frame"])):
        if off[o + 1] - off[o] >= 2:
            gap, bound = top2_gap(ref["score"], off, o), float(ref["score_bound"][off[o]:off[o + 1]].max())
            assert gap > 2 * bound, (name, o, gap, bound)


def check_head(name, heat, choice, score):
    """Shared by the CPU and the GPU test: results of one head call (numpy) against the referee of HEAD_CASES[name].

    Bounds (derived in weak_ref.sim_head's docstring from fp32 rounding, evaluated on the referee's fp64 values): every plane element
    within s_bound of the referee's plane OF THE CHOICE THE CODE MADE, every score within score_bound; the fixture has a top-2 gap
    above twice the score bound (asserted here), so the chosen index must equal the referee's."""
    case, ref = head_case(name)
    assert_fixture_gap(name)
    off = case["cand_off"]
    n_obj = len(case["obj_frame"])
    h, w = case["feat"].shape[1:3]
    assert heat.shape == (n_obj, h, w) and choice.shape == (n_obj,) and score.shape == (int(off[-1]),)
    if case["box"] is None:
        assert not score.any()
    else:
        err = np.abs(score.astype(np.float64) - ref["score"])
        print(name, "score err / bound", float((err / np.maximum(ref["score_bound"], 1e-300)).max()) if len(err) else 0.0)
        assert (err <= ref["score_bound"]).all(), (name, float(err.max()))
    if name in DEGENERATE:
        assert not score.any() and not ref["score"].any()
    assert choice.tolist() == ref["choice"].tolist(), name
    for o in range(n_obj):
        if off[o + 1] == off[o]:
            assert choice[o] == -1 and not heat[o].any(), (name, o)
            continue
        ci = int(off[o]) + int(choice[o])
        err = np.abs(heat[o].reshape(-1).astype(np.float64) - ref["s"][ci])
        print(name, o, "plane err / bound", float((err / ref["s_bound"][ci]).max()))
        assert (err <= ref["s_bound"][ci]).all(), (name, o, float(err.max()))


def head_inputs(name, device="cpu"):
    import torch
    case, _ = head_case(name)
    t = lambda k: None if case[k] is None else torch.from_numpy(case[k]).to(device)
    return t("feat"), t("obj_frame"), t("cand_off"), t("cand_xy"), t("box")
