"""Shared cases of the clip front end's tests (test_clip_front_cpu.py, test_clip_front_gpu.py).  The yardstick is Pillow itself:
Image.fromarray(hwc).resize((ow, oh), Image.BILINEAR) per frame, compared for exact equality."""
import functools
import random

import numpy as np
import torch
from PIL import Image

from ocpg_amd.datasets.clip_transforms import normalize_clip, resize_size
from ocpg_amd.datasets.targets import build_target

# (H, W, oh, ow, window or None); the window (top, left, h, w) is cropped first, as F.crop does, and then resized
GEOMETRIES = [
    (37, 53, 20, 29, None),              # fractional downscale, edge taps clipped
    (40, 70, 100, 175, None),            # upscale, 2 taps
    (97, 61, 12, 61, None),              # 19 taps; the horizontal pass is the identity
    (64, 64, 64, 33, None),              # the vertical pass is the identity
    (33, 47, 9, 13, None),
    (50, 50, 50, 50, None),
    (31, 57, 288, 530, None),
    (60, 80, 22, 31, (7, 5, 43, 60)),    # = crop((5, 7, 65, 50)).resize((31, 22))
]
CONTENTS = ("noise", "binary", "white")
TILE_CASE = (600, 40, 16, 40, None)      # 76 taps vertically: a 16-row tile does not fit the LDS the kernel asks for


@functools.lru_cache(maxsize=None)
def frames(t, h, w, content, seed=0):
    """-> uint8 [t, 3, h, w] (cached: treat as read-only)."""
    g = np.random.RandomState(seed + 1000 * t + 7 * h + w)
    if content == "noise":
        a = g.randint(0, 256, (t, 3, h, w))
    elif content == "binary":
        a = g.randint(0, 2, (t, 3, h, w)) * 255
    else:
        a = np.full((t, 3, h, w), 255)
    return torch.from_numpy(a.astype(np.uint8))


def pillow_resize(clip, out_hw, window=None):
    """uint8 [T, 3, H, W] -> uint8 [T, 3, oh, ow], every frame through Image.resize; a window is cropped beforehand with Image.crop."""
    oh, ow = out_hw
    out = []
    for f in clip:
        img = Image.fromarray(np.ascontiguousarray(f.permute(1, 2, 0).numpy()))
        if window is not None:
            top, left, h, w = window
            img = img.crop((left, top, left + w, top + h))
        out.append(torch.from_numpy(np.asarray(img.resize((ow, oh), Image.BILINEAR)).copy()).permute(2, 0, 1))
    return torch.stack(out).contiguous()


@functools.lru_cache(maxsize=None)
def pillow_case(t, geometry, content):
    h, w, oh, ow, window = geometry
    return pillow_resize(frames(t, h, w, content), (oh, ow), window)


def train_clip_and_target(t=2, h=40, w=60, seed=3):
    clip = frames(t, h, w, "noise", seed)
    g = torch.Generator().manual_seed(seed)
    masks = torch.zeros(t, h, w)
    for i in range(t):
        masks[i, 8 + i:30, 12:45 - i] = 1
    target = build_target(range(t), 5, masks, "the dog on the left of the right bench", weights=torch.rand(t, h, w, generator=g),
                          weak_masks=(torch.rand(t, h, w, generator=g) > 0.5).float())
    return clip, target


def pillow_train_pipeline(clip, seed, max_size=640, scales=(24, 28)):
    """train_pipeline's frames, step by step with Pillow, drawing from random.Random(seed) in the pipeline's order (select, scale(s),
    crop width then height, crop corner, flip) -> (normalised frames, {"cropped": bool, "flip": bool})."""
    r = random.Random(seed)
    cropped = not r.random() < 0.5
    if cropped:
        h, w = clip.shape[-2:]
        out_hw = resize_size(h, w, r.choice([400, 500, 600]), None)
        if out_hw != (h, w):
            clip = pillow_resize(clip, out_hw)
        hh, ww = clip.shape[-2:]
        cw = r.randint(384, min(ww, 600))
        ch = r.randint(384, min(hh, 600))
        i = 0 if hh == ch else r.randint(0, hh - ch)
        j = 0 if ww == cw else r.randint(0, ww - cw)
        clip = clip[:, :, i:i + ch, j:j + cw]
    size = r.choice(list(scales))
    h, w = clip.shape[-2:]
    out_hw = resize_size(h, w, size, max_size)
    if out_hw != (h, w):
        clip = pillow_resize(clip, out_hw)
    flip = r.random() < 0.5
    if flip:
        clip = clip.flip(-1)
    return normalize_clip(clip, None)[0], {"cropped": cropped, "flip": flip}


def assert_targets_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert a[k] == b[k], k
