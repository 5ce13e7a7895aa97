"""The clip front end on the CPU (models/ops/functions/clip_front_func.py, datasets/clip_transforms.py pil_exact=True,
util/misc.py:nested_tensor_from_u8_clips): the torch integer composition of Pillow's two 8-bit passes, against Pillow itself.
Every comparison is integer or bit equality."""
import random

import pytest
import torch
import torch.nn.functional as F

import clip_front_ref as R
from ocpg_amd.datasets.clip_transforms import (IMAGENET_MEAN, IMAGENET_STD, eval_pipeline, normalize_clip, resize_clip, resize_size,
                                               train_pipeline)
from ocpg_amd.models.ops.functions.clip_front_func import clip_front, resample_tables
from ocpg_amd.util.misc import nested_tensor_from_u8_clips, nested_tensor_from_videos_list

SEEDS = tuple(range(8))


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % g[:4])
def test_equals_pillow(geometry, content, t):
    h, w, oh, ow, window = geometry
    got = clip_front(R.frames(t, h, w, content), (oh, ow), window=window)
    assert got.dtype == torch.uint8 and torch.equal(got, R.pillow_case(t, geometry, content))


def test_tables_identity_pass_and_cache():
    bounds, coefs, ksize = resample_tables(50, 50)
    assert ksize == 3 and resample_tables(50, 50)[0] is bounds
    assert (bounds[:-1, 0] == range(49)).all() and (coefs[:, 0] == 1 << 22).all() and (coefs[:, 1:] == 0).all()
    _, _, ksize = resample_tables(97, 12)
    assert ksize == 19


@pytest.mark.parametrize("geometry", [R.GEOMETRIES[0], R.GEOMETRIES[1], R.GEOMETRIES[7]], ids=lambda g: "%dx%d-%dx%d" % g[:4])
def test_normalize_is_normalize_clip_of_pillow_bytes(geometry):
    h, w, oh, ow, window = geometry
    got = clip_front(R.frames(3, h, w, "noise"), (oh, ow), window=window, normalize=True)
    assert got.dtype == torch.float32 and torch.equal(got, normalize_clip(R.pillow_case(3, geometry, "noise"), None)[0])


@pytest.mark.parametrize("normalize", [False, True])
def test_flip(normalize):
    h, w, oh, ow, window = R.GEOMETRIES[7]
    src = R.frames(3, h, w, "noise")
    plain = clip_front(src, (oh, ow), window=window, normalize=normalize)
    assert torch.equal(clip_front(src, (oh, ow), window=window, flip=True, normalize=normalize), plain.flip(-1))


@pytest.mark.parametrize("normalize", [False, True])
def test_strided_out_fills_slot_only(normalize):
    h, w, oh, ow, window = R.GEOMETRIES[0]
    src = R.frames(2, h, w, "noise")
    sentinel = 77
    batch = torch.full((2, 3, 3, 32, 37), sentinel, dtype=torch.float32 if normalize else torch.uint8)
    ret = clip_front(src, (oh, ow), normalize=normalize, out=batch[1, :2, :, :oh, :ow])
    want = torch.full_like(batch, sentinel)
    want[1, :2, :, :oh, :ow] = clip_front(src, (oh, ow), normalize=normalize)
    assert torch.equal(batch, want) and ret.data_ptr() == batch[1].data_ptr()


def test_eval_pipeline_exact():
    clip = R.frames(2, 48, 86, "noise")
    oh, ow = resize_size(48, 86, 36, 64)
    assert (oh, ow) != (48, 86)
    out, target = eval_pipeline(size=36, max_size=64, pil_exact=True)(clip, None)
    x = R.pillow_resize(clip, (oh, ow)).to(torch.float32) / 255
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    assert target is None and torch.equal(out, (x - mean) / std)


def test_train_pipeline_exact_frames_and_targets():
    clip, target = R.train_clip_and_target()
    seen = set()
    for seed in SEEDS:
        want, info = R.pillow_train_pipeline(clip, seed)
        seen.add((info["cropped"], info["flip"]))
        got, got_t = train_pipeline(scales=(24, 28), pil_exact=True)(clip, dict(target), random.Random(seed))
        assert got.dtype == torch.float32 and torch.equal(got, want), (seed, info)
        _, default_t = train_pipeline(scales=(24, 28))(clip, dict(target), random.Random(seed))
        R.assert_targets_equal(got_t, default_t)
        assert tuple(got_t["size"].tolist()) == tuple(got.shape[-2:])
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen


def test_train_pipeline_exact_draws_as_the_default():
    """The generator is left in the same state: the same number of draws in the same order."""
    clip, target = R.train_clip_and_target()
    for seed in SEEDS:
        a, b = random.Random(seed), random.Random(seed)
        train_pipeline(scales=(24, 28), pil_exact=True)(clip, dict(target), a)
        train_pipeline(scales=(24, 28))(clip, dict(target), b)
        assert a.getstate() == b.getstate()


def test_resize_clip_exact_keeps_uint8_and_targets():
    clip, target = R.train_clip_and_target()
    out, t = resize_clip(clip, dict(target), 24, 640, pil_exact=True)
    _, t0 = resize_clip(clip, dict(target), 24, 640)
    assert out.dtype == torch.uint8 and torch.equal(out, R.pillow_resize(clip, resize_size(40, 60, 24, 640)))
    R.assert_targets_equal(t, t0)


def test_nested_tensor_from_u8_clips():
    a, b = R.frames(2, 40, 70, "noise"), R.frames(3, 33, 47, "noise")
    sizes, flips, windows = [(20, 35), (24, 30)], [False, True], [None, (2, 3, 30, 40)]
    got = nested_tensor_from_u8_clips([a, b], sizes, flips=flips, windows=windows)
    singles = [clip_front(c, s, window=w, flip=f, normalize=True) for c, s, f, w in zip((a, b), sizes, flips, windows)]
    assert torch.equal(singles[1], normalize_clip(R.pillow_resize(b, sizes[1], windows[1]).flip(-1), None)[0])
    want = nested_tensor_from_videos_list(singles, size_divisibility=32)
    assert got.tensors.shape == (2, 3, 3, 32, 64)
    assert torch.equal(got.tensors, want.tensors) and torch.equal(got.mask, want.mask) and got.mask._ocpg_key == want.mask._ocpg_key
    pad = got.mask[:, :, None].expand_as(got.tensors)
    assert bool((got.tensors[pad] == 0).all())


def test_errors():
    src = R.frames(1, 37, 53, "noise")
    with pytest.raises(ValueError, match="uint8"):
        clip_front(src.float(), (20, 29))
    for window in ((0, 0, 38, 53), (-1, 0, 10, 10), (30, 50, 7, 4), (0, 0, 0, 5)):
        with pytest.raises(ValueError, match="window"):
            clip_front(src, (20, 29), window=window)
    with pytest.raises(ValueError, match="out must be"):
        clip_front(src, (20, 29), out=torch.empty(1, 3, 20, 29))
    with pytest.raises(ValueError, match="uint8"):
        eval_pipeline(pil_exact=True)(src.float() / 255, None)
    clip, target = R.train_clip_and_target()
    with pytest.raises(ValueError, match="uint8"):
        train_pipeline(pil_exact=True)(clip.float() / 255, dict(target), random.Random(0))
    with pytest.raises(ValueError, match="uint8"):
        resize_clip(clip.float(), None, 24, pil_exact=True)


def test_writer_feeds_the_model_pillows_pixels(tmp_path):
    """write_expression_masks(pil_exact=True): the clip the model receives is normalize(Image.resize(decoded frame)), bit for bit."""
    import os

    from ocpg_amd import inference
    from ocpg_amd.datasets.video_folders import read_frames
    from test_datasets_cpu import _write_tiny_dataset
    root = str(tmp_path)
    names = _write_tiny_dataset(root)
    seen = []

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward_selected(self, clips, captions, targets):
            seen.append(clips[0].clone())
            t, _, h, w = clips[0].shape
            return {"pred_logits": torch.full((1, t, 1, 1), 3.0), "pred_masks_low": torch.full((1, t, h // 4, w // 4), -10.0), "mask_up": 4}

    n = inference.write_expression_masks(Stub(), root, "train", str(tmp_path / "out"), videos=["vidA"], native=True, pil_exact=True)
    raw = read_frames(os.path.join(root, "train", "JPEGImages", "vidA"), names)
    want = normalize_clip(R.pillow_resize(raw, resize_size(raw.shape[-2], raw.shape[-1], 360, 640)), None)[0]
    assert n == 2 * len(names) and len(seen) == 2 and all(torch.equal(s, want) for s in seen)


def test_default_eval_pipeline_unchanged():
    clip = R.frames(2, 48, 86, "noise")
    oh, ow = resize_size(48, 86, 36, 64)
    out, target = eval_pipeline(size=36, max_size=64)(clip, None)
    x = F.interpolate(clip.to(torch.float32) / 255.0, (oh, ow), mode="bilinear", align_corners=False, antialias=True)
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    assert target is None and torch.equal(out, (x - mean) / std)
    exact, _ = eval_pipeline(size=36, max_size=64, pil_exact=True)(clip, None)
    assert exact.shape == out.shape and not torch.equal(exact, out)        # the opt-in path is another function of the same clip
