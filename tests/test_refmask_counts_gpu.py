"""csrc/refmask_counts.hip on the MI355X through the C ABI (ocpg_refmask_counts_f32): its counts inside the bounds the float64 referee
of tests/mask_tail_ref.py leaves open (equal wherever the referee decides every pixel; tests/test_a2d_eval_cpu.py asserts the
properties of the seeded inputs), nothing written around the output and no dependence on what it held, argument errors, the binding
against the raw entry and against the ATen chain, and engine.evaluate_a2d on the fixture model."""
import pytest
import torch

import cases
import model_checks
import refmask_cases as C
from ocpg_amd.models.ops.functions import refmask_func

pytestmark = pytest.mark.gpu

LABEL_MISMATCH = 1e-4          # tests/test_mask_tail_gpu.py: the project's bound for kernel-vs-ATen decisions, as a share of the pixels


def _inputs(name, up, dev):
    samples = C.CASES[name][3]
    src = C.source(name, up).to(dev)
    geom = torch.tensor([list(c) + list(o) for c, o in samples], dtype=torch.int32)
    gt, off = refmask_func.pack_gt(C.ground_truth(name), dev)
    return src, geom, gt, off


def _call(src_t, up, geom_t, gt_t, off_t, counts_t, /, thr=C.THR, invert=0, max_out=None, **over):
    """The raw entry point on tensors (geometry and offsets on the host; copied to the device here); `over` replaces arguments by
    the header's names, to provoke argument errors (None = a NULL pointer)."""
    from ocpg_amd._lib import lib, stream_ptr
    b, q, hs, ws = src_t.shape
    geom_dev, off_dev = geom_t.to(src_t.device), off_t.to(src_t.device)
    mh, mw = max_out if max_out is not None else (int(geom_t[:, 2].max()), int(geom_t[:, 3].max()))
    a = {"src": src_t.data_ptr(), "B": b, "Q": q, "hs": hs, "ws": ws, "up": up, "geom_host": geom_t.data_ptr(), "geom": geom_dev.data_ptr(),
         "gt": gt_t.data_ptr(), "gt_off": off_dev.data_ptr(), "max_out_h": mh, "max_out_w": mw, "thr": thr, "invert": invert,
         "counts": counts_t.data_ptr()}
    a.update(over)
    rc = lib().ocpg_refmask_counts_f32(*a.values(), stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("up", C.UPS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_counts_inside_the_referee_bounds(dev, name, up):
    src, geom, gt, off = _inputs(name, up, dev)
    b, q = src.shape[:2]
    for invert in (0, 1):
        lo, hi = C.bounds(name, up, bool(invert))
        counts = torch.full((b, q, 3), -5, dtype=torch.int32, device=dev)
        assert _call(src, up, geom, gt, off, counts, invert=invert) == 0
        got = counts.cpu().long()
        print(f"{name} up {up} invert {invert}: {int((hi - lo).sum())} pixels open, counts {got[:, :, :2].flatten().tolist()}")
        assert torch.equal(got[..., 2], lo[..., 2])                                          # |G| exactly
        assert (lo <= got).all() and (got <= hi).all(), (lo - got).clamp(min=0).max().item()
    if name in C.ALL_NEGATIVE:
        i, j = C.ALL_NEGATIVE[name]
        oh, ow = C.CASES[name][3][i][1]
        assert got[i, j, 1] == oh * ow                                                        # with invert; without:
        assert _call(src, up, geom, gt, off, counts, invert=0) == 0 and counts[i, j, 1] == 0 and counts[i, j, 0] == 0
    if name in C.EMPTY_GT:
        assert (got[C.EMPTY_GT[name], :, 0] == 0).all() and (got[C.EMPTY_GT[name], :, 2] == 0).all()


def test_nothing_written_around_the_output_and_no_dependence_on_its_content(dev):
    src, geom, gt, off = _inputs("three-sizes", 4, dev)
    b, q = src.shape[:2]
    n = b * q * 3
    results = []
    for lead, sentinel in ((5, -77), (8, 123456)):                                            # 20- and 32-byte offsets into the allocation
        buf = torch.full((n + 16,), sentinel, dtype=torch.int32, device=dev)
        out = buf[lead:lead + n].view(b, q, 3)
        assert _call(src, 4, geom, gt, off, out, invert=1) == 0
        first = out.clone()
        assert _call(src, 4, geom, gt, off, out, invert=1) == 0                               # into the same, unzeroed buffer
        assert torch.equal(out, first)
        assert (buf[:lead] == sentinel).all() and (buf[lead + n:] == sentinel).all()
        results.append(first)
    assert torch.equal(results[0], results[1])
    # ground-truth planes that start off the 4-byte grid: byte offsets 1 and 3 into the packed buffer, same counts
    shifted = torch.zeros(gt.numel() + 8, dtype=torch.uint8, device=dev)
    for delta in (1, 3):
        shifted[delta:delta + gt.numel()] = gt
        out = torch.full((b, q, 3), -1, dtype=torch.int32, device=dev)
        assert _call(src, 4, geom, shifted, off + delta, out, invert=1) == 0
        assert torch.equal(out, results[0])


def test_argument_errors_leave_the_output_untouched(dev):
    src = torch.zeros(2, 3, 5, 7, device=dev)
    geom = torch.tensor([[20, 28, 10, 12], [18, 25, 9, 11]], dtype=torch.int32)
    gt = torch.ones(256, dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 120], dtype=torch.int64)
    counts = torch.full((2, 3, 3), -7, dtype=torch.int32, device=dev)

    def g(b, k, v):
        x = geom.clone()
        x[b, k] = v
        return x
    for kw in ({"B": 0}, {"Q": 0}, {"hs": 0}, {"ws": 0}, {"max_out_h": 0}, {"max_out_w": -1}):
        assert _call(src, 4, geom, gt, off, counts, **kw) == -1006, kw
    assert _call(src, 0, geom, gt, off, counts) == -1006
    for k in range(4):
        assert _call(src, 4, g(1, k, 0), gt, off, counts, max_out=(10, 12)) == -1006          # a non-positive geometry entry
    assert _call(src, 4, geom, gt, off, counts, invert=2) == -2301
    assert _call(src, 4, g(0, 0, 21), gt, off, counts) == -2302                               # crop_h > hs * up
    assert _call(src, 4, g(1, 1, 29), gt, off, counts) == -2302                               # crop_w > ws * up
    assert _call(src, 1, geom, gt, off, counts) == -2302
    huge = torch.tensor([[20, 28, 1 << 16, 1 << 15], [18, 25, 9, 11]], dtype=torch.int32)
    assert _call(src, 4, huge, gt, off, counts) == -2303                                      # out_h * out_w = 2^31
    assert _call(src, 4, geom, gt, off, counts, max_out=(9, 12)) == -2304                     # a sample taller than the stated maximum
    assert _call(src, 4, geom, gt, off, counts, max_out=(10, 11)) == -2304
    assert _call(src, 4, geom, gt, off, counts, geom_host=None) == -2305 and _call(src, 4, geom, gt, off, counts, geom=None) == -2305
    assert _call(src, 4, geom, gt, off, counts, gt=None) == -2306 and _call(src, 4, geom, gt, off, counts, gt_off=None) == -2306
    assert _call(src, 4, geom, gt, off, counts, max_out=(4 * 65535 + 1, 12)) == -1008         # refused before any launch
    assert _call(src, 4, geom, gt, off, counts, src=None) == -1001
    assert _call(src, 4, geom, gt, off, counts, counts=None) == -1015
    assert (counts == -7).all()
    # and the same sizes, valid, do write: logit 0 -> p = 0.5, not above the threshold
    assert _call(src, 4, geom, gt, off, counts) == 0
    want = torch.tensor([[0, 0, 120], [0, 0, 99]], dtype=torch.int32, device=dev)[:, None].expand(2, 3, 3)
    assert torch.equal(counts, want)
    assert _call(src, 4, geom, gt, off, counts, invert=1) == 0
    assert torch.equal(counts, torch.tensor([[120, 120, 120], [99, 99, 99]], dtype=torch.int32, device=dev)[:, None].expand(2, 3, 3))


@pytest.mark.parametrize("name,up", [("three-sizes", 4), ("rough", 1), ("wide", 1)])
def test_binding_against_the_raw_entry_and_the_aten_chain(dev, name, up):
    src, geom, gt, off = _inputs(name, up, dev)
    samples = C.CASES[name][3]
    crops, sizes, gts = [s[0] for s in samples], [s[1] for s in samples], C.ground_truth(name)
    for invert in (True, False):
        raw = torch.empty((*src.shape[:2], 3), dtype=torch.int32, device=dev)
        assert _call(src, up, geom, gt, off, raw, invert=int(invert)) == 0
        native = refmask_func.refmask_counts(src, up, crops, sizes, [g.to(dev) for g in gts], invert=invert, native=True)
        assert native.dtype == torch.int64 and torch.equal(native, raw.long())
        assert torch.equal(refmask_func.refmask_counts(src, up, crops, sizes, gts, invert=invert), native)      # default; masks from the host
        aten = refmask_func.refmask_counts(src, up, crops, sizes, [g.to(dev) for g in gts], invert=invert, native=False)
        assert aten.is_cuda and torch.equal(aten[..., 2], native[..., 2])
        pixels = torch.tensor([h * w for h, w in sizes], device=dev)[:, None, None]
        diff = (aten - native).abs()
        print(f"{name} up {up} invert {invert}: kernel vs ATen chain, largest count difference {int(diff.max())} pixels")
        assert (diff.double() <= LABEL_MISMATCH * pixels).all()


# ---- the driver --------------------------------------------------------------------------------------------------------------------
class _WithText(torch.nn.Module):
    """The fixture model behind the (samples, captions, targets) call of the evaluation loop: captions index precomputed text."""

    def __init__(self, model, texts):
        super().__init__()
        self.model, self.texts = model, texts

    def forward(self, samples, captions, targets):
        assert len(captions) == 1
        # as a list of clips the model pads to its own size divisibility (200 -> 208 columns here): the crop is a real one
        return self.model(list(samples.tensors), self.texts[int(captions[0])], targets)


def test_evaluate_a2d_on_the_fixture_model(golden, dev, monkeypatch):
    from ocpg_amd import _lib, engine, metrics
    from ocpg_amd.models import fallbacks
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    from ocpg_amd.util.misc import NestedTensor
    g = golden("infer_collate")
    m = g.meta
    model = model_checks.build_product(m, dev)[1].eval()
    f, s, pm = cases.tiny_text(1)
    net = _WithText(model, [PrecomputedText((f * a).to(dev), (s * b).to(dev), pm.to(dev)) for a, b in m["text_scale"]])
    frames = g["infer_frames"][:m["crop_len"]]
    h, w = int(frames.shape[-2]), int(frames.shape[-1])
    loader = []
    for i, orig in enumerate([(h * 2 + 3, w * 2 - 5), (h + 7, w + 30)]):
        gt = torch.zeros(orig, dtype=torch.bool)
        gt[orig[0] // 4:orig[0] // 4 * 3, orig[1] // 5:orig[1] // 5 * 3] = True
        t = {"caption": str(i), "image_id": f"v_{1 - i}_f_1_i_0", "size": torch.tensor([h, w]), "orig_size": torch.tensor(orig), "gt_mask": gt}
        loader.append((NestedTensor(frames[None].clone(), torch.zeros(1, frames.shape[0], h, w, dtype=torch.bool)), [t]))

    seen = {}
    add = metrics.RefMaskAccumulator.add

    def spy(self, image_ids, scores, counts, gt_area=None):
        seen.setdefault(seen["run"], []).append(torch.as_tensor(counts).cpu())
        return add(self, image_ids, scores, counts, gt_area)
    monkeypatch.setattr(metrics.RefMaskAccumulator, "add", spy)

    seen["run"] = "aten"
    before = fallbacks.snapshot()
    want = engine.evaluate_a2d(net, loader, dev, native=False)
    after_aten = fallbacks.snapshot()
    seen["run"] = "native"
    calls = _lib.census(True)
    try:
        got = engine.evaluate_a2d(net, loader, dev, native=True)
        assert calls.get("ocpg_refmask_counts_f32", 0) == len(loader)                         # one call per batch
    finally:
        _lib.census(False)
    # library_fallbacks: the counts step adds none -- the run makes exactly the fixture model's own, as the run without the kernel did
    after = fallbacks.snapshot()
    assert after.keys() == after_aten.keys()
    assert {k: v - before.get(k, 0) for k, v in after_aten.items()} == {k: v - after_aten[k] for k, v in after.items()}
    assert set(got) == set(metrics.AP_LABELS) | {"P@0.5", "P@0.6", "P@0.7", "P@0.8", "P@0.9", "overall_iou", "mean_iou"} == set(want)
    assert len(seen["native"]) == len(seen["aten"]) == len(loader)
    for (samples, targets), a, b in zip(loader, seen["native"], seen["aten"]):
        pixels = int(targets[0]["orig_size"].prod())
        assert torch.equal(a[..., 2], b[..., 2]) and a[0, 0, 2] == int(targets[0]["gt_mask"].sum())
        print(f"evaluate_a2d native vs ATen chain on {pixels} pixels: counts {a.flatten().tolist()} vs {b.flatten().tolist()}")
        assert ((a - b).abs().double() <= LABEL_MISMATCH * pixels).all()
