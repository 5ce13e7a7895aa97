"""ocpg_clip_front_u8 (csrc/clip_front.hip) on the GPU: against Pillow itself and against the CPU composition, bit for bit."""
import random

import pytest
import torch

import clip_front_ref as R
from ocpg_amd import _lib
from ocpg_amd.datasets.clip_transforms import eval_pipeline, train_pipeline
from ocpg_amd.models.ops.functions.clip_front_func import clip_front, device_tables, normalize_lut, tile_rows
from ocpg_amd.util.misc import nested_tensor_from_u8_clips

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % g[:4])
def test_equals_pillow(dev, geometry, content):
    h, w, oh, ow, window = geometry
    calls = _lib.census(True)
    got = clip_front(R.frames(3, h, w, content).to(dev), (oh, ow), window=window)
    _lib.census(False)
    assert calls == {"ocpg_clip_front_u8": 1}                    # the kernel, one launch
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), R.pillow_case(3, geometry, content))


def test_equals_pillow_realistic(dev):
    src = R.frames(2, 480, 854, "noise")
    got = clip_front(src.to(dev), (360, 640))
    assert torch.equal(got.cpu(), R.pillow_resize(src, (360, 640)))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("geometry", [R.GEOMETRIES[0], R.GEOMETRIES[6], R.GEOMETRIES[7]], ids=lambda g: "%dx%d-%dx%d" % g[:4])
def test_modes_and_flip_equal_cpu(dev, geometry, normalize, flip):
    h, w, oh, ow, window = geometry
    src = R.frames(3, h, w, "noise")
    got = clip_front(src.to(dev), (oh, ow), window=window, flip=flip, normalize=normalize)
    want = clip_front(src, (oh, ow), window=window, flip=flip, normalize=normalize)
    assert got.dtype == want.dtype and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_unaligned_window_and_destination(dev, normalize, flip):
    """Odd left edge of the window, out_w % 4 != 0, a destination that starts at an odd element of its buffer and whose rows are an odd
    number of elements apart: every packing decision is taken per group.  The buffer around the slot keeps its sentinel."""
    t, h, w, window, oh, ow, ph, pw = 2, 45, 90, (3, 7, 40, 77), 21, 71, 24, 75
    assert window[1] % 2 == 1 and ow % 4 != 0 and pw % 2 == 1
    src = R.frames(t, h, w, "noise")
    dtype = torch.float32 if normalize else torch.uint8

    def run(device):
        buf = torch.full((5 + t * 3 * ph * pw,), 99, dtype=dtype, device=device)
        slot = buf[1:1 + t * 3 * ph * pw].view(t, 3, ph, pw)[:, :, 2:2 + oh, 3:3 + ow]
        clip_front(src.to(device), (oh, ow), window=window, flip=flip, normalize=normalize, out=slot)
        return buf.cpu(), slot.cpu()

    buf, slot = run(dev)
    buf_cpu, slot_cpu = run("cpu")
    want = R.pillow_resize(src, (oh, ow), window)
    assert torch.equal(slot_cpu, clip_front(want, (oh, ow), flip=flip, normalize=normalize))      # identity resize: flip / normalise only
    assert torch.equal(buf, buf_cpu)
    assert int((buf == 99).sum()) >= buf.numel() - t * 3 * oh * ow


def test_small_tile_rows(dev):
    h, w, oh, ow, _ = R.TILE_CASE
    tr, rows = tile_rows(h, oh)
    assert tr < 16 and rows * 64 <= 32768 and tile_rows(480, 360)[0] == 16
    for content in R.CONTENTS:
        src = R.frames(2, h, w, content)
        assert torch.equal(clip_front(src.to(dev), (oh, ow)).cpu(), R.pillow_resize(src, (oh, ow))), content


def test_pipelines_equal_cpu(dev):
    clip = R.frames(2, 48, 86, "noise")
    got, _ = eval_pipeline(size=36, max_size=64, pil_exact=True)(clip.to(dev), None)
    want, _ = eval_pipeline(size=36, max_size=64, pil_exact=True)(clip, None)
    assert torch.equal(got.cpu(), want)
    clip, target = R.train_clip_and_target()
    for seed in range(4):                                         # both branches (the CPU test asserts the coverage of these seeds)
        got, got_t = train_pipeline(scales=(24, 28), pil_exact=True)(clip.to(dev), dict(target), random.Random(seed))
        want, want_t = train_pipeline(scales=(24, 28), pil_exact=True)(clip, dict(target), random.Random(seed))
        assert torch.equal(got.cpu(), want), seed
        R.assert_targets_equal(got_t, want_t)


def test_collate_equals_cpu(dev):
    a, b = R.frames(2, 40, 70, "noise"), R.frames(3, 33, 47, "noise")
    sizes, flips, windows = [(20, 35), (24, 30)], [False, True], [None, (2, 3, 30, 40)]
    got = nested_tensor_from_u8_clips([a.to(dev), b.to(dev)], sizes, flips=flips, windows=windows)
    want = nested_tensor_from_u8_clips([a, b], sizes, flips=flips, windows=windows)
    assert torch.equal(got.tensors.cpu(), want.tensors) and torch.equal(got.mask.cpu(), want.mask)


def test_graph_capture_and_replay(dev):
    h, w, oh, ow, window = R.GEOMETRIES[7]
    src = R.frames(3, h, w, "noise").to(dev)
    device_tables(window[2], oh, dev), device_tables(window[3], ow, dev), normalize_lut(dev)      # resident before the capture
    eager = clip_front(src, (oh, ow), window=window, flip=True, normalize=True)
    static = torch.zeros_like(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        clip_front(src, (oh, ow), window=window, flip=True, normalize=True, out=static)
    static.fill_(7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
