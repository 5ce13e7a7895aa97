"""The A2D-Sentences / JHMDB-Sentences evaluation from integer counts, on the CPU: metrics.coco_ap_single_gt against the plain-loop
referee of tests/coco_ap_ref.py and against hand-derived literals, refmask_counts' torch composition against the post-processor it
restates, engine.evaluate_a2d against engine.evaluate_referred_masks, the ground truth from the reference's JSON, two gloo ranks, and
the properties of the seeded inputs that tests/test_refmask_counts_gpu.py relies on."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import coco_ap_ref
import refmask_cases as C
from ocpg_amd import engine, metrics
from ocpg_amd.models.ops.functions.refmask_func import refmask_counts
from ocpg_amd.models.postprocessors import A2DSentencesPostProcess, rle_encode
from ocpg_amd.util.misc import NestedTensor

KEYS = set(metrics.AP_LABELS) | {"P@0.5", "P@0.6", "P@0.7", "P@0.8", "P@0.9", "overall_iou", "mean_iou"}


# ---- coco_ap_single_gt -------------------------------------------------------------------------------------------------------------
def _random_problem(seed, empty_range=None):
    """40 images x 5 queries: ground truths in every area range (but `empty_range`), tied scores within and across images, empty
    predictions, predictions larger and smaller than their range."""
    g = np.random.default_rng(seed)
    n, q = 40, 5
    sides = {"small": (6, 30), "medium": (34, 90), "large": (100, 160)}
    names = [k for k in sides if k != empty_range]
    counts = np.zeros((n, q, 3), dtype=np.int64)
    for i in range(n):
        lo, hi = sides[names[i % len(names)]]
        area = int(g.integers(lo, hi)) * int(g.integers(lo, hi))
        for j in range(q):
            pred = int(area * g.choice([0.0, 0.3, 0.8, 1.0, 1.3, 40.0]) * g.uniform(0.7, 1.0))
            inter = int(min(pred, area) * g.choice([0.0, 0.5, 0.9, 1.0]))
            counts[i, j] = (inter, pred, area)
    scores = g.choice(np.round(np.linspace(0.05, 0.95, 12), 3), size=(n, q)).astype(np.float32)       # 12 values for 200 detections
    scores[3] = scores[3, 0]                                                                           # one image, all tied
    counts[5, :, :2] = 0                                                                               # one image, nothing predicted
    return scores, counts


@pytest.mark.parametrize("empty_range", [None, "small", "medium", "large"])
def test_ap_equals_the_plain_loop_referee(empty_range):
    scores, counts = _random_problem(11, empty_range)
    assert len(np.unique(scores)) < scores.size / 4 and (counts[:, :, 1] == 0).any()
    area = counts[:, 0, 2]
    present = {"small": (area <= 1024).any(), "medium": ((area >= 1024) & (area <= 9216)).any(), "large": (area >= 9216).any()}
    assert all(v == (k != empty_range) for k, v in present.items())
    order = np.random.default_rng(1).permutation(len(scores))
    for kw in ({}, {"order": order}, {"gt_area": area * 0.9 + 3.0}):
        got = metrics.coco_ap_single_gt(scores, counts, **kw)
        want = coco_ap_ref.coco_ap(scores.astype(np.float64), counts, **kw)
        assert list(got) == list(metrics.AP_LABELS) == coco_ap_ref.LABELS
        for k in got:
            assert abs(got[k] - want[k]) <= 1e-12, (kw.keys(), k, got[k], want[k])
        assert 0.0 < got["mAP 0.5:0.95"] < 1.0
    if empty_range is not None:
        assert metrics.coco_ap_single_gt(scores, counts)["AP 0.5:0.95 " + empty_range[0].upper()] == -1.0
    # tensors are taken as well as arrays
    assert metrics.coco_ap_single_gt(torch.from_numpy(scores), torch.from_numpy(counts)) == metrics.coco_ap_single_gt(scores, counts)


def test_ap_hand_cases():
    ap = metrics.coco_ap_single_gt
    # perfect predictions, ground truths small and large only
    counts = np.array([[[100, 100, 100]], [[400, 400, 400]], [[10000, 10000, 10000]]])
    got = ap(np.array([[0.9], [0.8], [0.7]]), counts)
    # (to rounding: COCOeval's precision is TP / (TP + FP + spacing(1)), 1 - 2.2e-16 for a single true positive)
    assert got == pytest.approx({"mAP 0.5:0.95": 1.0, "AP 0.5": 1.0, "AP 0.75": 1.0, "AP 0.5:0.95 S": 1.0, "AP 0.5:0.95 M": -1.0,
                                 "AP 0.5:0.95 L": 1.0}, abs=1e-12, rel=0)
    assert got["AP 0.5:0.95 M"] == -1.0
    # one image, the top-scored query at IoU 0.77: matched at 0.5 .. 0.75 (six thresholds of ten)
    got = ap(np.array([[0.9, 0.2]]), np.array([[[77, 77, 100], [0, 50, 100]]]))
    assert abs(got["AP 0.5"] - 1.0) <= 1e-12 and abs(got["AP 0.75"] - 1.0) <= 1e-12 and abs(got["mAP 0.5:0.95"] - 0.6) <= 1e-12
    # one image, the top-scored query at IoU 0.3 and the second at 0.9: a false positive first, precision 1/2 at every recall
    # point for the nine thresholds up to 0.9, nothing at 0.95
    got = ap(np.array([[0.2, 0.9]]), np.array([[[90, 90, 100], [30, 30, 100]]]))
    assert abs(got["AP 0.5"] - 0.5) <= 1e-12 and abs(got["AP 0.75"] - 0.5) <= 1e-12 and abs(got["mAP 0.5:0.95"] - 0.45) <= 1e-12
    # a small ground truth; the top-scored detection misses it and is larger than `small`: ignored there, a false positive overall
    got = ap(np.array([[0.9, 0.5]]), np.array([[[0, 5000, 100], [100, 100, 100]]]))
    assert abs(got["AP 0.5:0.95 S"] - 1.0) <= 1e-12 and abs(got["mAP 0.5:0.95"] - 0.5) <= 1e-12
    assert got["AP 0.5:0.95 M"] == -1.0 and got["AP 0.5:0.95 L"] == -1.0
    # ... while one of the range's own size is not ignored
    got = ap(np.array([[0.9, 0.5]]), np.array([[[0, 500, 100], [100, 100, 100]]]))
    assert abs(got["AP 0.5:0.95 S"] - 0.5) <= 1e-12
    # an empty union counts as IoU 0 and the `area` of the JSON, not |G|, places the ground truth
    got = ap(np.array([[0.9]]), np.array([[[0, 0, 0]]]))
    assert got["mAP 0.5:0.95"] == 0.0
    got = ap(np.array([[0.9]]), np.array([[[100, 100, 100]]]), gt_area=[5000.0])
    assert got["AP 0.5:0.95 S"] == -1.0 and abs(got["AP 0.5:0.95 M"] - 1.0) <= 1e-12


def test_accumulator_follows_the_reference_rules():
    acc = metrics.RefMaskAccumulator()
    assert acc.summary() == {}
    # equal top scores: the LAST query wins (select_best_query); (I + 1e-6) / (U + 1e-6): two empty masks count as IoU 1
    acc.add(["b", "a"], np.array([[0.7, 0.7], [0.1, 0.6]], dtype=np.float32), np.array([[[0, 10, 10], [10, 10, 10]], [[5, 5, 5], [0, 0, 0]]]))
    acc.add(["b"], np.array([[0.9, 0.1]], dtype=np.float32), np.array([[[0, 1, 1], [0, 1, 1]]]))          # seen before: counts once
    s = acc.summary()
    assert set(s) == KEYS
    assert s["P@0.5"] == 1.0 and s["P@0.9"] == 1.0 and s["mean_iou"] == 1.0 and s["overall_iou"] == 1.0
    big = metrics.RefMaskAccumulator()
    big.add([0, 1], np.zeros((2, 1), dtype=np.float32), np.array([[[2 ** 30, 2 ** 31, 2 ** 31]], [[1, 3, 2 ** 31]]]))
    assert big.summary()["overall_iou"] == (2 ** 30 + 1) / (3 * 2 ** 30 + 2 ** 31 + 2)                      # int64 sums: exact


# ---- the composition against the post-processor ------------------------------------------------------------------------------------
def _smooth(shape, seed):
    import mask_tail_ref as R
    return R.logits(shape, "smooth", seed)


@pytest.mark.parametrize("invert", [True, False])
def test_composition_equals_the_post_processor(invert):
    sizes, origs = [(16, 24), (12, 20), (15, 17)], [(32, 48), (27, 40), (19, 23)]
    masks = _smooth((3 * 5, 16, 24), 21).view(3, 5, 16, 24)
    gts = [torch.rand(o, generator=torch.Generator().manual_seed(i)) > 0.6 for i, o in enumerate(origs)]
    out = {"pred_logits": torch.zeros(3, 1, 5, 1), "pred_masks": masks[:, None]}
    post = A2DSentencesPostProcess()(out, torch.tensor(origs), torch.tensor(sizes))
    got = refmask_counts(masks, 1, sizes, origs, gts, invert=invert)
    assert got.dtype == torch.int64 and got.shape == (3, 5, 3)
    for b, (p, g) in enumerate(zip(post, gts)):
        pred = p["masks"][:, 0] if invert else ~p["masks"][:, 0]
        _, inter, union = metrics.mask_iou(pred, g[None].expand_as(pred))
        area = pred.flatten(1).sum(1)
        assert torch.equal(got[b, :, 0], inter.long()) and torch.equal(got[b, :, 1], area)
        assert torch.equal(got[b, :, 1] + got[b, :, 2] - got[b, :, 0], union.long())
        assert (got[b, :, 2] == g.sum()).all()
    assert 0.1 < (got[..., 1].sum() / sum(5 * h * w for h, w in origs)).item() < 0.9
    # tensors for the sizes, uint8 masks
    again = refmask_counts(masks, 1, torch.tensor(sizes), torch.tensor(origs), [g.to(torch.uint8) * 255 for g in gts], invert=invert)
    assert torch.equal(again, got)
    # up 4: the nearest replication the model's eval branch applies
    low = _smooth((3 * 5, 4, 6), 22).view(3, 5, 4, 6)
    up = low.repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert torch.equal(refmask_counts(low, 4, sizes, origs, gts, invert=invert), refmask_counts(up, 1, sizes, origs, gts, invert=invert))
    with pytest.raises(RuntimeError, match="GPU"):
        refmask_counts(masks, 1, sizes, origs, gts, native=True)
    with pytest.raises(ValueError):
        refmask_counts(masks, 1, [(17, 24)] * 3, origs, gts)
    with pytest.raises(ValueError):
        refmask_counts(masks, 1, sizes, origs, gts[::-1])


@pytest.mark.parametrize("name", list(C.CASES))
def test_inputs_of_the_gpu_count_test(name):
    """What tests/test_refmask_counts_gpu.py takes for granted about the seeded cases, and the composition inside the same bounds."""
    for up in C.UPS:
        set_, total = 0, 0
        for want, decided in C.expectation(name, up):
            open_share = 1 - decided.flatten(1).double().mean(1)
            assert open_share.max().item() <= 5e-3, (name, up, open_share)
            set_, total = set_ + int(want.sum()), total + want.numel()
        assert 0.1 <= set_ / total <= 0.9, (name, up, set_ / total)
        (vh, vw), q, kind, samples, seed = C.CASES[name]
        for invert in (False, True):
            lo, hi = C.bounds(name, up, invert)
            got = refmask_counts(C.source(name, up), up, [s[0] for s in samples], [s[1] for s in samples], C.ground_truth(name), invert=invert)
            assert (lo <= got).all() and (got <= hi).all(), (name, up, invert)
    for g in C.ground_truth(name):
        assert g.sum() == 0 or 0.1 <= g.double().mean().item() <= 0.9
    if name in C.EMPTY_GT:
        assert C.ground_truth(name)[C.EMPTY_GT[name]].sum() == 0
    if name in C.ALL_NEGATIVE:
        i, j = C.ALL_NEGATIVE[name]
        assert all((C.source(name, up)[i, j] < 0).all() and not C.expectation(name, up)[i][0][j].any() and C.expectation(name, up)[i][1][j].all()
                   for up in C.UPS)


def test_at_least_two_gpu_cases_decide_every_pixel():
    exact = [(n, up) for n in C.CASES for up in C.UPS if all(bool(d.all()) for _, d in C.expectation(n, up))]
    print("every pixel decided:", exact)
    assert len(exact) >= 2


# ---- the driver --------------------------------------------------------------------------------------------------------------------
Q = 5
PAD = (16, 24)
SAMPLES = [  # image_id, augmented size, original size: ids out of order, sizes all different
    ("v_2_f_7_i_0", (16, 24), (32, 48)), ("v_1_f_3_i_1", (12, 20), (27, 40)), ("v_3_f_1_i_0", (15, 17), (19, 23)), ("v_0_f_9_i_2", (9, 24), (40, 31))]


class Stub(torch.nn.Module):
    """Stands in for the model, as in tests/test_datasets_cpu.py: seeded mask logits and scores per sample, looked up by the number
    the loader writes into the clip's first pixel."""

    def forward(self, samples, captions, targets):
        idx = [int(v) for v in samples.tensors[:, 0, 0, 0, 0].tolist()]
        masks = torch.stack([_smooth((Q,) + PAD, 300 + i) for i in idx])[:, None]
        logits = torch.stack([torch.randn(Q, 1, generator=torch.Generator().manual_seed(400 + i)) for i in idx])[:, None]
        for k, i in enumerate(idx):
            if i != 2:
                logits[k, 0, i % Q] = 3.0                              # the query the ground truth was made from scores highest
        return {"pred_logits": logits, "pred_masks": masks}


def _gt_mask(i):
    h, w = SAMPLES[i][2]
    m = torch.zeros(h, w, dtype=torch.bool)
    post = A2DSentencesPostProcess()({"pred_logits": torch.zeros(1, 1, Q, 1), "pred_masks": _smooth((Q,) + PAD, 300 + i)[None, None]},
                                     torch.tensor([SAMPLES[i][2]]), torch.tensor([SAMPLES[i][1]]))
    m |= post[0]["masks"][i % Q, 0]                                   # one query's own mask, shifted: IoUs spread over (0, 1)
    return torch.roll(m, (i, 2 * i), (0, 1))


def _loader(batches=((0, 1), (2,), (3,))):
    out = []
    for idx in batches:
        x = torch.zeros(len(idx), 1, 3, *PAD)
        targets = []
        for k, i in enumerate(idx):
            x[k, 0, 0, 0, 0] = i
            image_id, size, orig = SAMPLES[i]
            targets.append({"caption": "x", "image_id": image_id, "size": torch.tensor(size), "orig_size": torch.tensor(orig), "gt_mask": _gt_mask(i)})
        out.append((NestedTensor(x, torch.zeros(len(idx), 1, *PAD, dtype=torch.bool)), targets))
    return out


def test_driver_against_evaluate_referred_masks():
    want = engine.evaluate_referred_masks(Stub(), _loader(), A2DSentencesPostProcess(), "cpu")
    got = engine.evaluate_a2d(Stub(), _loader(), "cpu")
    assert set(got) == KEYS and set(want) < KEYS
    for k in want:                                                    # the older loop sums in fp32
        assert abs(got[k] - want[k]) <= 1e-6, (k, got[k], want[k])
    assert 0.0 < got["mean_iou"] < 1.0 and 0.0 < got["P@0.5"] < 1.0   # a spread of IoUs, not a degenerate case
    for k in metrics.AP_LABELS[:3]:
        assert 0.0 <= got[k] <= 1.0
    # the AP numbers are those of the referee on the post-processor's own masks
    scores, counts = [], []
    for samples, targets in _loader():
        out = Stub()(samples, None, targets)
        post = A2DSentencesPostProcess()(out, torch.stack([t["orig_size"] for t in targets]), torch.stack([t["size"] for t in targets]))
        for p, t in zip(post, targets):
            m, g = p["masks"][:, 0], t["gt_mask"]
            scores.append(p["scores"].double().numpy())
            counts.append(np.stack([(m & g).flatten(1).sum(1).numpy(), m.flatten(1).sum(1).numpy(), np.full(Q, int(g.sum()))], 1))
    ids = [s[0] for s in SAMPLES]
    ref = coco_ap_ref.coco_ap(scores, counts, order=sorted(range(len(ids)), key=lambda i: ids[i]))
    for k in metrics.AP_LABELS:
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    assert engine.evaluate_a2d(Stub(), [], "cpu") == {}


def test_ground_truth_from_the_coco_json(tmp_path):
    anns = []
    for i, (image_id, _, _) in enumerate(SAMPLES):
        m = _gt_mask(i)
        rle = rle_encode(m)
        anns.append({"id": i, "image_id": image_id, "category_id": 1, "iscrowd": 0, "area": float(m.sum()),
                     "segmentation": {"size": rle["size"], "counts": rle["counts"].decode("ascii")}})
    path = tmp_path / "a2d_sentences_test_annotations_in_coco_format.json"
    path.write_text(json.dumps({"categories": [{"id": 1, "name": "dummy_class"}], "images": [{"id": a["image_id"]} for a in anns], "annotations": anns}))
    gt = metrics.load_coco_gt(str(path))
    assert list(gt) == [s[0] for s in SAMPLES]
    for i, (image_id, _, orig) in enumerate(SAMPLES):
        mask, area = gt[image_id]
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == orig and torch.equal(mask.bool(), _gt_mask(i)) and area == float(_gt_mask(i).sum())
    want = engine.evaluate_a2d(Stub(), _loader(), "cpu")
    stripped = [(s, [{k: v for k, v in t.items() if k != "gt_mask"} for t in ts]) for s, ts in _loader()]
    assert engine.evaluate_a2d(Stub(), stripped, "cpu", gt=str(path)) == want
    assert engine.evaluate_a2d(Stub(), stripped, "cpu", gt=gt) == want
    # the JSON's area field, not the mask's, sorts a ground truth into its range
    anns[0]["area"] = 1e6
    path.write_text(json.dumps({"annotations": anns}))
    assert engine.evaluate_a2d(Stub(), stripped, "cpu", gt=str(path)) != want


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(2)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    batches = _loader()
    mine = batches[1:] if rank == 0 else batches[:1]                  # rank order != image order
    q.put((rank, engine.evaluate_a2d(Stub(), mine, "cpu")))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_return_the_single_process_numbers():
    want = engine.evaluate_a2d(Stub(), _loader(), "cpu")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=200) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0] == got[1]
    assert set(got[0]) == KEYS
    for k in want:                                                    # the mean over another order of the same four numbers
        assert abs(got[0][k] - want[k]) <= 1e-12, (k, got[0][k], want[k])
