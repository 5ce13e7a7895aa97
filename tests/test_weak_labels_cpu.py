"""The weak-annotation generator on the host (ocpg_amd/weak_labels.py, ops/functions/sim_heat_func.py) against tests/weak_ref.py:
centres and boxes exactly, candidate lists exactly, the torch composition of the similarity head within fp32 bounds of the fp64
referee, and a dataset tree from frames and masks to files the training loader reads."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import weak_ref as R


def _blobs(seed, n, h, w):
    g = np.random.default_rng(seed)
    out = np.zeros((n, h, w), dtype=bool)
    yy, xx = np.ogrid[:h, :w]
    for m in out:
        for _ in range(int(g.integers(1, 4))):
            y, x, r = int(g.integers(0, h)), int(g.integers(0, w)), int(g.integers(1, 12))
            m |= (yy - y) ** 2 + (xx - x) ** 2 <= r * r
    return out


def _mask(h, w, *rects):
    m = np.zeros((h, w), dtype=bool)
    for y0, y1, x0, x1 in rects:
        m[y0:y1, x0:x1] = True
    return m


CENTER_MASKS = {
    "single_pixel": [_mask(9, 13, (4, 5, 6, 7))],
    "full_row": [_mask(9, 13, (3, 4, 0, 13))],
    "rect_11x7_plateau": [_mask(15, 21, (2, 9, 5, 16))],
    "two_blobs_one_on_edge": [_mask(20, 30, (0, 6, 0, 5), (9, 18, 12, 27))],
    "l_shape": [_mask(24, 24, (3, 20, 4, 9), (15, 20, 4, 21))],
    "random_blobs_37x83": list(_blobs(5, 6, 37, 83)),
    "empty": [_mask(9, 13)],
    "empty_among_others": [_mask(12, 12, (2, 7, 3, 9)), _mask(12, 12), _mask(12, 12, (0, 12, 0, 11))],
}


@pytest.mark.parametrize("name", list(CENTER_MASKS))
def test_centers_and_boxes_equal_the_sequential_two_pass(name):
    from ocpg_amd.weak_labels import mask_centers_and_boxes
    masks = np.stack(CENTER_MASKS[name])
    want = [R.center_and_box(m) for m in masks]
    for as_type in (torch.bool, torch.float32):
        centers, boxes, valid = mask_centers_and_boxes(torch.from_numpy(masks).to(as_type))
        assert centers.dtype == boxes.dtype == valid.dtype == torch.int64
        assert torch.equal(centers, torch.tensor([c for c, _, _ in want], dtype=torch.int64).view(-1, 2)), name
        assert torch.equal(boxes, torch.tensor([b for _, b, _ in want], dtype=torch.int64).view(-1, 4)), name
        assert torch.equal(valid, torch.tensor([v for _, _, v in want], dtype=torch.int64)), name
    if name.startswith("empty"):
        assert 0 in valid.tolist()


def test_distance_transform_equals_the_sequential_two_pass_everywhere():
    """Not only the arg-max: every pixel of the batched row sweep equals the per-pixel recurrence."""
    from ocpg_amd.weak_labels import chamfer_distance_5x5
    masks = _blobs(11, 4, 23, 31)
    got = chamfer_distance_5x5(torch.from_numpy(masks))
    for m, d in zip(masks, got):
        assert d.tolist() == R.chamfer_5x5(m.tolist())


def test_mask_without_background_has_no_centre():
    from ocpg_amd.weak_labels import mask_centers_and_boxes
    with pytest.raises(ValueError):
        mask_centers_and_boxes(torch.ones(1, 6, 8, dtype=torch.bool))
    with pytest.raises(ValueError):
        R.center_and_box(np.ones((6, 8), dtype=bool))


@pytest.mark.parametrize("box,frame,fmap", [
    ((100, 100, 101, 101), (720, 1280), (23, 40)),          # one cell
    ((0, 0, 1279, 719), (720, 1280), (23, 40)),             # the whole map: 920 cells, the stride must grow
    ((64, 64, 65, 90), (720, 1280), (23, 40)),              # x ends coincide after scaling
    ((3, 7, 900, 500), (720, 1280), (45, 80)),
    ((17, 5, 300, 359), (360, 640), (12, 20)),
])
def test_candidate_lists_equal_the_referee(box, frame, fmap):
    from ocpg_amd.weak_labels import box_candidates, point_cell
    cur, cells = box_candidates(box, frame, fmap)
    want_cur, want_cells = R.box_candidates(box, frame, fmap)
    assert list(cur) == want_cur and [tuple(c) for c in cells] == want_cells
    assert 1 <= len(cells) <= 256
    if box == (0, 0, 1279, 719):
        assert len(cells) < 23 * 40 and cells[1][0] == cells[0][0] and cells[1][1] > cells[0][1] + 1      # strided, y inner
    assert point_cell((box[2], box[3]), frame, fmap) == R.point_cell((box[2], box[3]), frame, fmap)


@pytest.mark.parametrize("name", list(R.HEAD_CASES))
def test_composition_within_fp32_bounds_of_the_fp64_referee(name):
    from ocpg_amd.models.ops.functions.sim_heat_func import sim_heat
    heat, choice, score = sim_heat(*R.head_inputs(name), native=False)
    assert heat.dtype == torch.float32 and choice.dtype == torch.int32 and score.dtype == torch.float32
    R.check_head(name, heat.numpy(), choice.numpy(), score.numpy())


def test_head_refuses_what_it_cannot_serve():
    from ocpg_amd.models.ops.functions.sim_heat_func import sim_heat
    feat, obj_frame, off, xy, box = R.head_inputs("2x3x8_two")
    with pytest.raises(RuntimeError, match="GPU"):
        sim_heat(feat, obj_frame, off, xy, box, native=True)                  # no quiet fall-back when the kernel is asked for
    with pytest.raises(ValueError):
        sim_heat(feat, obj_frame, off.flip(0), xy, box)
    with pytest.raises(ValueError):
        sim_heat(feat, obj_frame, off, xy + 5, box)


class _StandInBody(nn.Module):
    """A seeded stride-32 conv stack in place of the ResNet body: same interface ({"0": [F, C, H/32, W/32]}), no bias and no
    non-linearity, so features of different cells point in unrelated directions."""

    def __init__(self, channels=16, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        chans = [3, 8, 8, 8, 8, channels]
        self.convs = nn.ModuleList(nn.Conv2d(a, b, 3, stride=2, padding=1, bias=False) for a, b in zip(chans, chans[1:]))
        for c in self.convs:
            with torch.no_grad():
                c.weight.copy_(torch.randn(c.weight.shape, generator=g) / (c.weight[0].numel() ** 0.5))

    def forward(self, x):
        for c in self.convs:
            x = c(x)
        return {"0": x}


def stand_in_labeler(channels=16, native=None):
    from ocpg_amd.weak_labels import SimilarityLabeler
    lab = SimilarityLabeler("resnet50", frames_per_pass=3, native=native)
    lab.body = _StandInBody(channels)
    return lab.eval()


def _write_tree(root, n_frames=4, h=96, w=128):
    """Two videos, two objects named by the expressions; object 2 is missing from vidB (an invisible object in every frame)."""
    from PIL import Image
    g = np.random.default_rng(0)
    meta, exps = {"videos": {}}, {"videos": {}}
    names = ["%05d" % (5 * i) for i in range(n_frames)]
    for v in ("vidA", "vidB"):
        for sub in ("JPEGImages", "Annotations"):
            os.makedirs(os.path.join(root, "train", sub, v), exist_ok=True)
        for i, n in enumerate(names):
            Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "train", "JPEGImages", v, n + ".jpg"))
            lab = np.zeros((h, w), dtype=np.uint8)
            lab[8:40, 6 + 2 * i:50 + 2 * i] = 1
            if v == "vidA":
                lab[70:90, 80:120] = 2
            ann = Image.fromarray(lab)
            ann.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * 759)
            ann.save(os.path.join(root, "train", "Annotations", v, n + ".png"))
        meta["videos"][v] = {"objects": {"1": {"category": "zebra"}, "2": {"category": "ape"}}}
        exps["videos"][v] = {"frames": names, "expressions": {"0": {"exp": "the zebra on the left", "obj_id": "1"},
                                                              "1": {"exp": "an ape", "obj_id": "2"},
                                                              "2": {"exp": "a striped animal", "obj_id": "1"}}}
    os.makedirs(os.path.join(root, "meta_expressions", "train"), exist_ok=True)
    with open(os.path.join(root, "train", "meta.json"), "w") as f:
        json.dump(meta, f)
    with open(os.path.join(root, "meta_expressions", "train", "meta_expressions.json"), "w") as f:
        json.dump(exps, f)
    return names


def test_dataset_tree_round_trip(tmp_path):
    """Frames + masks -> .npz weak annotations -> the training dataset reads them; a second run touches nothing."""
    from ocpg_amd.datasets import ClipPipeline, check_target
    from ocpg_amd.datasets import clip_transforms as ct
    from ocpg_amd.datasets.targets import weak_targets_from_heatmaps
    from ocpg_amd.datasets.video_folders import RefVideoClips, default_weak_loader
    from ocpg_amd.weak_labels import write_weak_annotations
    root = str(tmp_path)
    names = _write_tree(root)
    labeler = stand_in_labeler()
    assert write_weak_annotations(root, "train", labeler) == 2 * len(names)
    weak = os.path.join(root, "train", "AnnotationsWeakly")
    files = sorted(os.path.join(d, f) for d, _, fs in os.walk(weak) for f in fs)
    assert [os.path.relpath(f, weak) for f in files] == [os.path.join(v, n + ".npz") for v in ("vidA", "vidB") for n in names]
    z = np.load(files[0])
    assert z["obj_ids"].tolist() == [1, 2] and z["heatPoint"].shape == (2, 3, 4) and z["heatBBox"].shape == (2, 3, 4)
    assert z["centerPoint"].shape == (2, 2) and z["heatPoint"].dtype == np.float32
    cx, cy = z["centerPoint"][0]
    assert 6 <= cx < 50 and 8 <= cy < 40                                                 # inside object 1's rectangle
    # the visible object's weak mask is not empty, the invisible one's planes are zero
    heat, ids = default_weak_loader(weak)("vidA", names[0])
    assert ids == [1, 2]
    for k in range(2):
        m, _ = weak_targets_from_heatmaps(heat, k)
        assert float(m.sum()) > 0, k
    zb = np.load(os.path.join(weak, "vidB", names[0] + ".npz"))
    assert zb["heatPoint"][0].any() and not zb["heatPoint"][1].any() and not zb["heatBBox"][1].any()
    assert zb["centerPoint"][1].tolist() == [0, 0]
    small = ClipPipeline([lambda c, t, r: ct.resize_clip(c, t, 32, 64), lambda c, t, r: (c, check_target(t)), lambda c, t, r: ct.normalize_clip(c, t)])
    ds = RefVideoClips(root, "train", 3, small, supervision="box", seed=7)
    x, t = ds[0]
    assert x.shape[:2] == (3, 3) and t["weak_masks"].shape == t["masks"].shape and float(t["weak_masks"].sum()) > 0
    # a second run skips every frame
    before = {f: (os.stat(f).st_mtime_ns, open(f, "rb").read()) for f in files}
    assert write_weak_annotations(root, "train", labeler) == 0
    assert {f: (os.stat(f).st_mtime_ns, open(f, "rb").read()) for f in files} == before
    assert sorted(os.path.join(d, f) for d, _, fs in os.walk(weak) for f in fs) == files


def test_label_frames_matches_the_referee_head(tmp_path):
    """label_frames = features + host-built candidate lists + the head: its planes equal the referee's on the same features."""
    from ocpg_amd.weak_labels import mask_centers_and_boxes
    labeler = stand_in_labeler(channels=12)
    g = torch.Generator().manual_seed(1)
    frames = torch.randn(2, 3, 160, 224, generator=g)
    masks = torch.zeros(2, 2, 160, 224, dtype=torch.bool)
    masks[0, 0, 20:120, 30:200] = True
    masks[1, 0, 60:70, 100:110] = True
    masks[1, 1, 0:160, 0:100] = True
    centers, boxes, valid = (v.view(2, 2, -1) for v in mask_centers_and_boxes(masks.flatten(0, 1)))
    valid = valid.view(2, 2)
    hp, hb = labeler.label_frames(frames, centers, boxes, valid)
    feat = labeler.features(frames).numpy()
    h, w = feat.shape[1:3]
    assert hp.shape == hb.shape == (2, 2, h, w) == (2, 2, 5, 7)
    assert not hp[0, 1].any() and not hb[0, 1].any()                                      # the invisible object
    for f, o in ((0, 0), (1, 0), (1, 1)):
        cell = R.point_cell(centers[f, o].tolist(), (160, 224), (h, w))
        ref = R.sim_head(feat, [f], [0, 1], [cell])
        assert (np.abs(hp[f, o].reshape(-1).numpy() - ref["s"][0]) <= ref["s_bound"][0]).all()
        cur, cells = R.box_candidates(boxes[f, o].tolist(), (160, 224), (h, w))
        ref = R.sim_head(feat, [f], [0, len(cells)], cells, [cur])
        near_best = np.nonzero(ref["score"] >= ref["score"].max() - 2 * ref["score_bound"].max())[0]
        err = [np.abs(hb[f, o].reshape(-1).numpy() - ref["s"][c]) <= ref["s_bound"][c] for c in near_best]
        assert any(e.all() for e in err), (f, o)
