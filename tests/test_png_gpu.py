"""csrc/png_rle.hip on the MI355X: the files png_encode makes from device planes equal the host composition's byte for byte (which
tests/test_png_cpu.py pins to the bit-at-a-time restatement), through the binding and through the C ABI into guarded outputs; shapes
that move the row addresses, fill the bit buffer or make the largest sums; the census; the refusals; and the writers on the
infer_collate model.  Every comparison is exact."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import cases
import model_checks
import png_ref as R
from ocpg_amd.models.ops.functions import png_func as F
from test_png_cpu import check_file

pytestmark = pytest.mark.gpu

PLANES = R.edge_planes()
GUARD = 64                      # bytes around every output


def _guarded(nbytes, dev):
    buf = torch.full((nbytes + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _raw(planes, slack=0):
    """ocpg_png_rle_count + ocpg_png_rle_emit into outputs pre-filled with 0xEE -> (streams, adlers); everything around them and
    `slack` bytes behind the last stream must keep the fill."""
    from ocpg_amd._lib import lib, stream_ptr
    n, h, w = planes.shape
    dev = planes.device
    ws = torch.full((24 * n * h,), 0xEE, dtype=torch.uint8, device=dev)
    t_buf, totals = _guarded(24 * n, dev)
    assert lib().ocpg_png_rle_count(planes.data_ptr(), n, h, w, ws.data_ptr(), totals.data_ptr(), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((t_buf[:GUARD] == 0xEE).all() and (t_buf[-GUARD:] == 0xEE).all())
    host = totals.cpu().view(torch.int64).view(n, 3)
    sizes = host[:, 0].tolist()
    cap = sum(sizes) + slack
    o_buf, out = _guarded(cap, dev)
    assert lib().ocpg_png_rle_emit(planes.data_ptr(), n, h, w, ws.data_ptr(), host.data_ptr(), out.data_ptr(), cap, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((o_buf[:GUARD] == 0xEE).all() and (o_buf[GUARD + sum(sizes):] == 0xEE).all())
    data = out.cpu().numpy()
    streams, at = [], 0
    for s in sizes:
        streams.append(data[at:at + s].tobytes())
        at += s
    return streams, [F.adler_from_sums(h * (w + 1), s0, s1) for _, s0, s1 in host.tolist()]


def _same_as_host(planes, dev, palette=None):
    """png_encode on the device against png_encode on the host, and the Pillow / zlib checks of the file."""
    got = F.png_encode(planes.to(dev), palette)
    want = F.png_encode(planes, palette)
    assert got == want
    return got


@pytest.mark.parametrize("name", list(PLANES))
def test_edge_planes_byte_for_byte(dev, name):
    plane = PLANES[name]
    data, = _same_as_host(plane, dev)
    check_file(data, plane)
    streams, adlers = _raw(plane[None].to(dev), slack=5)
    assert streams == [F.deflate_rle(plane.numpy())]
    assert data == F._frame(plane.shape[0], plane.shape[1], None, streams[0], adlers[0])


def test_batch_of_three_and_palette(dev):
    batch = R.batch_planes()
    for data, plane in zip(_same_as_host(batch, dev), batch):
        check_file(data, plane)
    streams, _ = _raw(batch.to(dev))
    assert streams == [F.deflate_rle(p.numpy()) for p in batch]
    labels = torch.stack([R.label_plane(), R.label_plane().flip(1)])
    for data, plane in zip(_same_as_host(labels, dev, R.PALETTE), labels):
        check_file(data, plane, R.PALETTE)


def test_rows_of_854_bytes_at_every_address_residue(dev):
    """W = 854: row addresses are no multiples of 4; the planes themselves start 0..3 bytes into an allocation."""
    g = torch.Generator().manual_seed(21)
    planes = (torch.rand((3, 9, 854), generator=g) < 0.3).to(torch.uint8) * 255
    planes[1, :, 400:] = torch.randint(0, 256, (9, 454), dtype=torch.uint8, generator=g)
    planes[2, 4:] = 0
    want = F.png_encode(planes)
    for data, plane in zip(want, planes):
        check_file(data, plane)
    for shift in range(4):
        buf = torch.zeros(planes.numel() + 8, dtype=torch.uint8, device=dev)
        view = buf[shift:shift + planes.numel()].view(planes.shape)
        view.copy_(planes)
        assert view.is_contiguous() and view.data_ptr() % 4 == (buf.data_ptr() + shift) % 4
        assert F.png_encode(view) == want


def test_all_literals_and_the_widest_row(dev):
    """64 x 64 random bytes: every token a literal.  2 x 4096 of alternating 255 / 254: the longest stream a row can have, 9 bits per
    byte, which fills the per-wave bit buffer; a random binary row of the same width next to it."""
    g = torch.Generator().manual_seed(22)
    noise = torch.randint(0, 256, (64, 64), dtype=torch.uint8, generator=g)
    data, = _same_as_host(noise, dev)
    check_file(data, noise)
    wide = torch.tensor([255, 254], dtype=torch.uint8).repeat(2, 2048)
    assert wide.shape[1] == F.MAX_WIDTH
    data, = _same_as_host(wide, dev)
    check_file(data, wide)
    assert len(F.deflate_rle(wide.numpy())) == 2 * ((3 + 8 + 9 * 4096 + 10 + 7) // 8 + 4) + 2
    binary = (torch.rand((3, 4096), generator=g) < 0.3).to(torch.uint8) * 255
    binary[2] = 0
    data, = _same_as_host(binary, dev)
    check_file(data, binary)


def test_full_size_planes(dev):
    """720 x 1280: all-zero (the file is at most 16 KB: the rule gives 11.6 KB, a literal-only coder about 920 KB) and all-255 (the
    largest Adler sums, S1 about 1.1e14, and 9-bit literals); both must decode."""
    zero = torch.zeros(720, 1280, dtype=torch.uint8)
    data, = _same_as_host(zero, dev)
    print(f"all-zero 720 x 1280: {len(data)} bytes")
    assert len(data) <= 16 * 1024
    Image.open(io.BytesIO(data)).verify()
    assert not np.array(Image.open(io.BytesIO(data))).any()
    full = torch.full((720, 1280), 255, dtype=torch.uint8)
    data, = _same_as_host(full, dev)
    Image.open(io.BytesIO(data)).verify()
    img = Image.open(io.BytesIO(data))
    assert img.mode == "L" and bool((np.array(img) == 255).all()) and np.array(img).shape == (720, 1280)


def test_the_same_entries_for_one_plane_and_for_five(dev):
    """Two entries per call, whatever N: count (two launches: rows, per-plane scan) and emit (one launch)."""
    from ocpg_amd import _lib
    g = torch.Generator().manual_seed(23)
    planes = ((torch.rand((5, 33, 130), generator=g) < 0.3).to(torch.uint8) * 255).to(dev)
    seen = []
    for n in (1, 5):
        calls = _lib.census(True)
        try:
            files = F.png_encode(planes[:n])
        finally:
            _lib.census(False)
        assert len(files) == n
        seen.append(dict(calls))
    assert seen[0] == seen[1] == {"ocpg_png_rle_count": 1, "ocpg_png_rle_emit": 1}
    assert sum(seen[1].values()) <= 3


def test_refusals_leave_the_outputs_alone(dev):
    from ocpg_amd._lib import lib, stream_ptr
    wide = torch.zeros(1, 2, F.MAX_WIDTH + 1, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        F.png_encode(wide)
    ok = torch.zeros(2, 6, 10, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        F.png_encode(ok.transpose(1, 2))
    with pytest.raises(ValueError):
        F.png_encode(ok[:, :, ::2])
    ws = torch.full((24 * 2 * 6 + 8,), 0xEE, dtype=torch.uint8, device=dev)
    totals = torch.full((2 * 24 + 8,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full((4096,), 0xEE, dtype=torch.uint8, device=dev)
    good = torch.tensor([[40, 0, 0], [40, 0, 0]], dtype=torch.int64)
    negative, huge = torch.tensor([[40, 0, 0], [-1, 0, 0]], dtype=torch.int64), torch.tensor([[40, 0, 0], [10 ** 6, 0, 0]], dtype=torch.int64)
    s = stream_ptr()
    L = lib()
    count = [
        (-2701, (wide.data_ptr(), 1, 2, F.MAX_WIDTH + 1, ws.data_ptr(), totals.data_ptr(), s)),
        (-1006, (ok.data_ptr(), 0, 6, 10, ws.data_ptr(), totals.data_ptr(), s)),
        (-1006, (ok.data_ptr(), 2, 6, 0, ws.data_ptr(), totals.data_ptr(), s)),
        (-2702, (ok.data_ptr(), 65536, 6, 10, ws.data_ptr(), totals.data_ptr(), s)),
        (-2702, (ok.data_ptr(), 2, 65536, 10, ws.data_ptr(), totals.data_ptr(), s)),
        (-2702, (ok.data_ptr(), 1024, 4097, 10, ws.data_ptr(), totals.data_ptr(), s)),
        (-1001, (None, 2, 6, 10, ws.data_ptr(), totals.data_ptr(), s)),
        (-2703, (ok.data_ptr(), 2, 6, 10, None, totals.data_ptr(), s)),
        (-2703, (ok.data_ptr(), 2, 6, 10, ws.data_ptr() + 4, totals.data_ptr(), s)),
        (-2704, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), None, s)),
        (-2704, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), totals.data_ptr() + 4, s)),
    ]
    for code, args in count:
        assert L.ocpg_png_rle_count(*args) == code, code
    emit = [
        (-2701, (wide.data_ptr(), 1, 2, F.MAX_WIDTH + 1, ws.data_ptr(), good.data_ptr(), out.data_ptr(), 4096, s)),
        (-1006, (ok.data_ptr(), 2, 0, 10, ws.data_ptr(), good.data_ptr(), out.data_ptr(), 4096, s)),
        (-1001, (None, 2, 6, 10, ws.data_ptr(), good.data_ptr(), out.data_ptr(), 4096, s)),
        (-2703, (ok.data_ptr(), 2, 6, 10, ws.data_ptr() + 2, good.data_ptr(), out.data_ptr(), 4096, s)),
        (-2705, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), None, out.data_ptr(), 4096, s)),
        (-2705, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), negative.data_ptr(), out.data_ptr(), 4096, s)),
        (-2705, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), huge.data_ptr(), out.data_ptr(), 4096, s)),
        (-2706, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), good.data_ptr(), None, 4096, s)),
        (-2706, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), good.data_ptr(), out.data_ptr(), 79, s)),
        (-2706, (ok.data_ptr(), 2, 6, 10, ws.data_ptr(), good.data_ptr(), out.data_ptr(), 0, s)),
    ]
    for code, args in emit:
        assert L.ocpg_png_rle_emit(*args) == code, code
    torch.cuda.synchronize()
    for t in (ws, totals, out):
        assert bool((t == 0xEE).all())


class _Selected(torch.nn.Module):
    """The fixture model behind the string captions of the writer: 'zebra' is the first precomputed text, anything else the second."""

    def __init__(self, model, texts):
        super().__init__()
        self.model, self.texts = model, texts

    def _text(self, captions):
        return self.texts[0 if "zebra" in captions[0].lower() else 1]

    def forward(self, clips, captions, targets):
        return self.model(clips, self._text(captions), targets)

    def forward_selected(self, clips, captions, targets):
        return self.model.forward_selected(clips, self._text(captions), targets)


def test_writer_on_the_fixture_model(golden, dev, tmp_path, monkeypatch):
    """write_expression_masks(native=True) on the infer_collate model: png="native" hands mask_binary's device tensor to the kernels
    (the census shows both entries once per expression) and writes the files png="pil" writes, pixel for pixel.  The eval forward
    is not reproducible to the last bit from one call to the next, so the second writer call receives the
    first one's stride-4 logits again; the tail, the threshold and the encoders run both times."""
    from ocpg_amd import _lib, inference
    from ocpg_amd.datasets.clip_transforms import eval_pipeline
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    from test_datasets_cpu import _write_tiny_dataset
    g = golden("infer_collate")
    m = g.meta
    model = model_checks.build_product(m, dev)[1].eval()
    f, s, pm = cases.tiny_text(1)
    net = _Selected(model, [PrecomputedText((f * a).to(dev), (s * b).to(dev), pm.to(dev)) for a, b in m["text_scale"]])
    root = str(tmp_path / "data")
    names = _write_tiny_dataset(root, videos=("vidA",), n_frames=3, h=97, w=131)
    pipe = eval_pipeline(size=160, max_size=224)
    inner, kept = inference._selected_clips, {}

    def once(model, frames, expression, clip_len, amp_dtype):
        if expression not in kept:
            kept[expression] = inner(model, frames, expression, clip_len, amp_dtype)
        return kept[expression]
    monkeypatch.setattr(inference, "_selected_clips", once)
    pil, own = str(tmp_path / "pil"), str(tmp_path / "own")
    n_pil = inference.write_expression_masks(net, root, "train", pil, native=True, transform=pipe)
    calls = _lib.census(True)
    try:
        n_own = inference.write_expression_masks(net, root, "train", own, native=True, transform=pipe, png="native")
    finally:
        _lib.census(False)
    assert calls.get("ocpg_png_rle_count", 0) == 2 == calls.get("ocpg_png_rle_emit", 0)      # two expressions
    assert n_pil == n_own == 2 * len(names)
    seen = set()
    for exp in ("0", "1"):
        for name in names:
            rel = os.path.join("Annotations", "vidA", exp, name + ".png")
            a, b = Image.open(os.path.join(pil, rel)), Image.open(os.path.join(own, rel))
            assert a.mode == b.mode == "L" and b.size == (131, 97)
            assert np.array_equal(np.asarray(a), np.asarray(b))
            seen |= set(np.unique(np.asarray(b)).tolist())
    assert seen <= {0, 255} and len(kept) == 2
