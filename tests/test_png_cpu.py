"""models/ops/functions/png_func.py off the GPU: the vectorised host composition of the run-length PNG stream (DESIGN.md section
4.8sc) against the bit-at-a-time restatement of tests/png_ref.py, byte for byte, against zlib and against Pillow; the argument
errors; and the writers' png="native" switch on the stand-in model of tests/test_datasets_cpu.py.  Every comparison is exact."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R
from ocpg_amd.models.ops.functions import png_func as F

PLANES = R.edge_planes()


def check_file(data, plane, palette=None):
    """One PNG file against the plane it was made from: the naive restatement's bytes, zlib, Pillow."""
    plane = plane.numpy()
    assert data == R.png(plane, palette)
    kinds = [k for k, _ in R.chunks(data)]
    assert kinds == ([b"IHDR", b"PLTE", b"IDAT", b"IEND"] if palette is not None else [b"IHDR", b"IDAT", b"IEND"])
    idat = dict(R.chunks(data))[b"IDAT"]
    assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == R.filtered(plane)          # decompress checks Adler-32 too
    Image.open(io.BytesIO(data)).verify()
    img = Image.open(io.BytesIO(data))
    assert img.mode == ("P" if palette is not None else "L") and img.size == (plane.shape[1], plane.shape[0])
    assert np.array_equal(np.array(img), plane)
    if palette is not None:
        assert img.getpalette()[:len(palette)] == list(palette)


def test_the_edge_planes_cover_what_they_claim():
    rows = {p.shape[1] + 1 for p in PLANES.values()}
    assert {2, 3, 4, 257, 258, 259, 260, 516, 517, 519} <= rows
    assert any(p.shape == (1, 1) for p in PLANES.values()) and any(p.shape[0] == 1 and p.shape[1] > 1 for p in PLANES.values())
    assert any(p.shape[1] == 1 and p.shape[0] > 1 for p in PLANES.values())
    values = set(torch.cat([p.flatten() for p in PLANES.values()]).tolist())
    assert values == set(range(256))
    assert any(int(p[0, 0]) == 0 for p in PLANES.values()) and any(int(p[0, 0]) != 0 for p in PLANES.values())
    q = PLANES["repeated_row"]
    assert torch.equal(q[2], q[1]) and not torch.equal(q[1], q[0])
    a = PLANES["alternating"]
    assert bool((a[:, 1:] != a[:, :-1]).all()) and int(a[0, 0]) == 0                      # only the filter byte joins a run
    assert bool((PLANES["all_255"] == 255).all())


@pytest.mark.parametrize("name", list(PLANES))
def test_host_path_is_the_naive_stream(name):
    plane = PLANES[name]
    data, = F.png_encode(plane)
    check_file(data, plane)
    assert F.deflate_rle(plane.numpy()) == R.deflate(plane.numpy())


def test_a_batch_of_three_planes_and_a_two_dimensional_argument():
    batch = R.batch_planes()
    files = F.png_encode(batch)
    assert len(files) == 3 and len(set(files)) == 3
    for data, plane in zip(files, batch):
        check_file(data, plane)
    assert F.png_encode(batch[1]) == [files[1]]


def test_palette_file():
    plane = R.label_plane()
    data, = F.png_encode(plane, R.PALETTE)
    check_file(data, plane, R.PALETTE)
    full = [c % 256 for c in range(768)]
    data, = F.png_encode(plane, full)
    check_file(data, plane, full)


def test_adler_from_sums_is_zlib_adler():
    g = torch.Generator().manual_seed(11)
    for n in (1, 2, 5552, 5553, 70000):
        for d in (torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g), torch.full((n,), 255, dtype=torch.uint8)):
            v = d.numpy().astype(object)
            s0, s1 = int(v.sum()), int((np.arange(n, dtype=object) * v).sum())
            assert F.adler_from_sums(n, s0, s1) == zlib.adler32(d.numpy().tobytes())
    # the sums of an all-255 720 x 1280 plane (S1 about 1.1e14) in closed form, against zlib
    h, w = 720, 1280
    n = h * (w + 1)
    row = w * (w + 1) // 2                                                                 # sum of the positions 1..w of a row
    s0, s1 = 255 * h * w, 255 * (h * row + (w + 1) * w * (h * (h - 1) // 2))
    assert s1 > 10 ** 14
    filtered = np.full((h, w + 1), 255, dtype=np.uint8)
    filtered[:, 0] = 0
    assert F.adler_from_sums(n, s0, s1) == zlib.adler32(filtered.tobytes())


def test_argument_errors():
    ok = torch.zeros(2, 3, 4, dtype=torch.uint8)
    for bad in (ok.float(), ok.bool(), ok.to(torch.int8), ok[None], ok[0, 0], torch.zeros(0, 3, 4, dtype=torch.uint8), ok.numpy()):
        with pytest.raises(ValueError):
            F.png_encode(bad)
    for palette in ([0, 0], [0] * 4, [0] * 771, [0, 0, 256], [], [0, -1, 0]):
        with pytest.raises(ValueError):
            F.png_encode(ok, palette)
    assert len(F.png_encode(ok, [0] * 768)) == 2
    assert len(F.png_encode(ok.transpose(1, 2))) == 2                                      # a host tensor may be a view


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, files in os.walk(folder) for f in files)


def test_writers_native_switch_writes_the_same_files(tmp_path):
    """write_expression_masks / write_label_maps with png="native" against png="pil" (the default): same file set, same return
    value, same pixels and modes, the palette kept."""
    from ocpg_amd import inference
    from test_datasets_cpu import _write_tiny_dataset
    root = str(tmp_path / "data")
    names = _write_tiny_dataset(root)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, clips, captions, targets):
            t, _, h, w = clips[0].shape
            masks = torch.full((1, t, 2, h, w), -10.0)
            if "zebra" in captions[0].lower():
                masks[:, :, 1, : h // 2] = 10.0
            else:
                masks[:, :, 0, :, : w // 4] = 10.0
            logits = torch.tensor([[-3.0], [3.0]] if "zebra" in captions[0].lower() else [[3.0], [-3.0]]).expand(1, t, 2, 1)
            return {"pred_logits": logits, "pred_masks": masks}

        def forward_selected(self, clips, captions, targets):
            t, _, h, w = clips[0].shape
            low = torch.full((1, t, h // 4, w // 4), -10.0)
            if "zebra" in captions[0].lower():
                low[:, :, : h // 8] = 10.0
            else:
                low[:, :, :, : w // 16] = 10.0
            return {"pred_logits": torch.full((1, t, 1, 1), 3.0), "pred_masks_low": low, "mask_up": 4}

    for native in (False, True):
        pil, own = str(tmp_path / f"pil{native}"), str(tmp_path / f"own{native}")
        n_pil = inference.write_expression_masks(Stub(), root, "train", pil, videos=["vidA"], native=native)
        n_own = inference.write_expression_masks(Stub(), root, "train", own, videos=["vidA"], native=native, png="native")
        assert n_pil == n_own == 2 * len(names)
        assert _tree(pil) == _tree(own) and len(_tree(own)) == n_own
        for rel in _tree(own):
            a, b = Image.open(os.path.join(pil, rel)), Image.open(os.path.join(own, rel))
            assert a.mode == b.mode == "L" and np.array_equal(np.asarray(a), np.asarray(b))
            plane = torch.from_numpy(np.asarray(b).copy())
            assert open(os.path.join(own, rel), "rb").read() == R.png(plane.numpy())
        assert {int(v) for rel in _tree(own) for v in np.unique(np.asarray(Image.open(os.path.join(own, rel))))} == {0, 255}
    with pytest.raises(ValueError):
        inference.write_expression_masks(Stub(), root, "train", str(tmp_path / "x"), videos=["vidA"], png="zlib")

    labels = torch.stack([R.label_plane(), R.label_plane().flip(0), torch.zeros_like(R.label_plane())])
    for palette in (None, [7, 8, 9] * 4):
        pil, own = str(tmp_path / f"lab_pil{palette is None}"), str(tmp_path / f"lab_own{palette is None}")
        inference.write_label_maps(labels, pil, palette)
        inference.write_label_maps(labels, own, palette, png="native")
        assert _tree(pil) == _tree(own) == ["00000.png", "00001.png", "00002.png"]
        for rel, lab in zip(_tree(own), labels):
            a, b = Image.open(os.path.join(pil, rel)), Image.open(os.path.join(own, rel))
            assert a.mode == b.mode == "P" and np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), lab.numpy())
            want = palette if palette is not None else inference.label_palette()
            assert b.getpalette()[:len(want)] == want and a.getpalette()[:len(want)] == want
    with pytest.raises(ValueError):
        inference.write_label_maps(labels, str(tmp_path / "y"), png="zlib")
