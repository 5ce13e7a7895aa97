"""csrc/mask_tail.hip on the MI355X through the C ABI (ocpg_mask_tail_f32), against the float64 referee of tests/mask_tail_ref.py
at its elementwise bound; the decisions of modes 1 / 2 exactly wherever the referee can decide them; argument errors; the model
path (OCPG.forward_selected, native segment_video / segment_objects) against forward and the reference's arrays; one graph capture.
"""
import pytest
import torch
import torch.nn.functional as F

import cases
import mask_tail_ref as R
import model_checks

pytestmark = pytest.mark.gpu

# tests/test_model_gpu.py:869
ATOL_LOGITS, ATOL_MASKS, LABEL_MISMATCH = 2e-4, 5e-4, 1e-4


def _call(src, up, crop, out_size, mode, out, thr=0.5, bg=0.1, on_value=255, k=None, n=None, hs=None, ws=None):
    """The raw entry point on a [K, N, hs, ws] device tensor; sizes can be overridden to provoke argument errors."""
    from ocpg_amd._lib import lib, stream_ptr
    K, N, HS, WS = src.shape
    rc = lib().ocpg_mask_tail_f32(src.data_ptr(), K if k is None else k, N if n is None else n, HS if hs is None else hs,
                                  WS if ws is None else ws, up, crop[0], crop[1], out_size[0], out_size[1], mode, thr, bg, on_value,
                                  out.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_probabilities_against_fp64_at_the_bound(dev, idx):
    shape, up, crop, out_size, kind = R.CASES[idx]
    src = R.logits(shape, kind, 100 + idx)
    ref = R.referee(src, up, crop, out_size)
    # an odd element offset into the allocation: rows and the buffer itself start off the 16-byte grid
    buf = torch.full((shape[0] * out_size[0] * out_size[1] + 8,), -7.0, device=dev)
    for off in (0, 1):
        buf.fill_(-7.0)
        out = buf[off:off + shape[0] * out_size[0] * out_size[1]].view(shape[0], *out_size)
        assert _call(src.to(dev)[None], up, crop, out_size, 0, out) == 0
        got = out.cpu().double()
        ratio = ((got - ref["p"]).abs() / ref["bound_p"]).max().item()
        print(f"{R.case_id(R.CASES[idx])} offset {off}: at {ratio:.3f} of the probability bound")
        assert ratio <= 1.0
        assert (buf[:off] == -7.0).all() and (buf[off + out.numel():] == -7.0).all()         # nothing written around the output
        if up == 1 and tuple(crop) == tuple(out_size):
            assert (got - torch.sigmoid(src.double())).abs().max().item() <= 4 * R.EPS32
        if kind == "saturated":
            flat = ref["v"].abs() > 90                                  # away from the +100 / -100 transitions
            assert torch.isfinite(got).all() and flat.any() and ((got == 0) | (got == 1))[flat].all()


@pytest.mark.parametrize("idx", range(len(R.BINARY_CASES)), ids=[R.case_id(c) for c in R.BINARY_CASES])
def test_binary_decisions(dev, idx):
    case = R.BINARY_CASES[idx]
    shape, up, crop, out_size, kind = case
    src = R.logits(shape, kind, 100 + R.CASES.index(case))
    want, ok = R.binary_decision(R.referee(src, up, crop, out_size), 0.5)
    assert 1 - ok.double().mean().item() <= 5e-3
    assert 0.1 <= want[ok].double().mean().item() <= 0.9
    numel = shape[0] * out_size[0] * out_size[1]
    for on, off in ((255, 0), (1, 3)):
        buf = torch.full((numel + 8,), 77, dtype=torch.uint8, device=dev)
        out = buf[off:off + numel].view(shape[0], *out_size)
        assert _call(src.to(dev)[None], up, crop, out_size, 1, out, thr=0.5, on_value=on) == 0
        got = out.cpu()
        assert ((got == 0) | (got == on)).all()
        assert torch.equal(got[ok], want[ok].to(torch.uint8) * on)
        assert (buf[:off] == 77).all() and (buf[off + numel:] == 77).all()


@pytest.mark.parametrize("idx", range(len(R.LABEL_CASES)))
def test_label_decisions(dev, idx):
    k, shape, up, crop, out_size, seed = R.LABEL_CASES[idx]
    src = R.label_sources(k, shape, seed)
    want, ok = R.label_decision(R.referee(src, up, crop, out_size), 0.3, 0.1)
    assert 1 - ok.double().mean().item() <= 5e-3
    assert torch.bincount(want[ok].long(), minlength=k + 1).min().item() > 0          # every label, background included
    numel = shape[0] * out_size[0] * out_size[1]
    for off in (0, 1):
        buf = torch.full((numel + 8,), 77, dtype=torch.uint8, device=dev)
        out = buf[off:off + numel].view(shape[0], *out_size)
        assert _call(src.to(dev), up, crop, out_size, 2, out, thr=0.3, bg=0.1) == 0
        got = out.cpu()
        assert (got <= k).all() and torch.equal(got[ok], want[ok])
        assert (buf[:off] == 77).all() and (buf[off + numel:] == 77).all()


def test_label_tie_goes_to_the_lower_index(dev):
    k, shape, up, crop, out_size, seed = R.LABEL_CASES[1]
    src = R.label_sources(2, shape, seed)
    src = torch.cat([src, src[1:]], 0)                                  # objects 2 and 3: the same map
    want, ok = R.label_decision(R.referee(src, up, crop, out_size), 0.3, 0.1)
    assert (want == 2)[ok].any() and not (want == 3).any()
    out = torch.full((shape[0], *out_size), 77, dtype=torch.uint8, device=dev)
    assert _call(src.to(dev), up, crop, out_size, 2, out, thr=0.3, bg=0.1) == 0
    got = out.cpu()
    assert not (got == 3).any() and torch.equal(got[ok], want[ok])


def test_argument_errors_leave_the_output_untouched(dev):
    src1 = torch.zeros(1, 2, 5, 7, device=dev)
    src2 = torch.zeros(2, 2, 5, 7, device=dev)
    big = torch.zeros(256, 1, 2, 2, device=dev)
    f32 = torch.full((2, 10, 10), -7.0, device=dev)
    u8 = torch.full((2, 10, 10), 77, dtype=torch.uint8, device=dev)
    crop, size = (20, 28), (10, 10)
    assert _call(src2, 4, crop, size, 0, f32) == -2101                  # K != 1, mode 0
    assert _call(src2, 4, crop, size, 1, u8) == -2101                   # K != 1, mode 1
    assert _call(src1, 4, (21, 28), size, 0, f32) == -2102              # crop_h > hs * up
    assert _call(src1, 4, (20, 29), size, 1, u8) == -2102               # crop_w > ws * up
    assert _call(src1, 1, (5, 8), size, 2, u8) == -2102
    assert _call(big, 1, (2, 2), (10, 10), 2, u8[:1]) == -2103          # K > 255
    assert _call(src1, 4, crop, size, 3, u8) == -2104                   # no such mode
    assert _call(src1, 4, crop, size, 1, u8, on_value=256) == -2105
    for kw in ({"n": 0}, {"k": 0}, {"hs": 0}, {"ws": 0}):
        assert _call(src1, 4, crop, size, 0, f32, **kw) == -1006
    assert _call(src1, 0, crop, size, 0, f32) == -1006
    assert _call(src1, 4, (0, 28), size, 0, f32) == -1006 and _call(src1, 4, crop, (10, 0), 1, u8) == -1006
    assert _call(src1, 4, crop, (4 * 65535 + 1, 1), 1, u8) == -1008     # refused before any launch: out is never addressed
    assert (f32 == -7.0).all() and (u8 == 77).all()
    # and the same sizes, valid, do write
    assert _call(src1, 4, crop, size, 0, f32) == 0 and (f32 == 0.5).all()


def test_mask_labels_replays_from_a_captured_graph(dev):
    from ocpg_amd.models.ops.functions.mask_tail_func import mask_labels
    k, shape, up, crop, out_size, seed = R.LABEL_CASES[1]
    src = R.label_sources(k, shape, seed).to(dev)
    eager = mask_labels(src, up, crop, out_size, 0.3, 0.1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        static = mask_labels(src, up, crop, out_size, 0.3, 0.1)
    static.fill_(77)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert static.dtype == torch.uint8 and torch.equal(static, eager)


# ---- the model path ----------------------------------------------------------------------------------------------------------------
def _texts(meta, device):
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    f, s, pm = cases.tiny_text(1)
    return [PrecomputedText((f * a).to(device), (s * b).to(device), pm.to(device)) for a, b in meta["text_scale"]]


def _models(golden, dev, strict):
    """The infer_collate model; under OCPG_STRICT_HIP=1 a 256-channel model of the same depth from seeded initial weights instead: the
    fixture's 64 channels give the text gate 8 heads of 8 channels, which only library attention serves and strict mode refuses."""
    g = golden("infer_collate")
    if not strict:
        return model_checks.build_product(g.meta, dev)[1].eval()
    from ocpg_amd.models import build_model
    torch.manual_seed(0)
    model, _, _ = build_model(cases.default_args(device=str(dev), **dict(g.meta["cfg"], hidden_dim=256, mask_dim=256, dim_feedforward=256)))
    return model.to(dev).eval()


@pytest.mark.parametrize("strict", [False, True], ids=["fixture-model", "hidden-256-strict"])
def test_best_query_masks_are_the_eval_branch_bit_for_bit(golden, dev, monkeypatch, strict):
    """From ONE trunk evaluation, pred_masks_low replicated x4 IS the eval branch's pred_masks and the head outputs are its head
    outputs, torch.equal: the controller ran on the same rows for both, csrc/dynmask.hip evaluates a parameter set independently of
    how many share the launch (36 sets or 720), and MSO sees the same [t, 16, h, w] input.  Two separate forwards are compared in the
    next test: the ResNet body's result moves in its last bits from one call to the next, whichever path follows it."""
    from ocpg_amd.models import amp_cache, fallbacks
    g = golden("infer_collate")
    m = g.meta
    if strict:
        monkeypatch.setenv("OCPG_STRICT_HIP", "1")
        fallbacks.reset()
    model = _models(golden, dev, strict)
    frames = g["infer_frames"][:m["crop_len"]].to(dev)
    text = _texts(m, dev)[1]
    targets = [{"size": torch.as_tensor([int(frames.shape[-2]), int(frames.shape[-1])], device=dev)}]
    with torch.no_grad(), amp_cache.scope(model):
        trunk = model._trunk([frames], text, targets)
        full = model._all_masks(trunk, targets)
        sel = model._best_query_masks(trunk, targets)
    assert sel["mask_up"] == 4 and tuple(sel["pred_masks_low"].shape[:2]) == (1, frames.shape[0])
    for k in ("pred_logits", "pred_boxes", "reference_points"):
        assert torch.equal(sel[k], full[k]), k
    up = F.interpolate(sel["pred_masks_low"], scale_factor=4)[:, :, None]
    assert up.shape == full["pred_masks"].shape
    assert torch.equal(up, full["pred_masks"]), (up - full["pred_masks"]).abs().max().item()
    assert full["pred_masks"].std().item() > 1e-3                      # a map, not a constant
    if strict:
        assert fallbacks.snapshot() == {}


def test_forward_selected_against_forward(golden, dev):
    """Two separate forwards.  They cannot be compared bit for bit: the eval forward itself is not reproducible from one call to the
    next (the ResNet body's convolutions, before anything this path touches).  The bound is the project's
    own for mask logits in fp32 (model_checks.MASK_LOGIT_ATOL, 1e-3) and test_model_gpu.py:869's 2e-4 for the head outputs."""
    g = golden("infer_collate")
    m = g.meta
    model = _models(golden, dev, False)
    frames = g["infer_frames"][:m["crop_len"]].to(dev)
    text = _texts(m, dev)[1]
    targets = [{"size": torch.as_tensor([int(frames.shape[-2]), int(frames.shape[-1])], device=dev)}]
    with torch.no_grad():
        full = model([frames], text, targets)
        sel = model.forward_selected([frames], text, targets)
    assert set(sel) == {"pred_logits", "pred_boxes", "reference_points", "pred_masks_low", "mask_up"}
    for k in ("pred_logits", "pred_boxes", "reference_points"):
        assert sel[k].shape == full[k].shape and (sel[k] - full[k]).abs().max().item() <= ATOL_LOGITS, k
    up = F.interpolate(sel["pred_masks_low"], scale_factor=4)[:, :, None]
    err = (up - full["pred_masks"]).abs().max().item()
    print(f"forward_selected vs forward, separate calls: mask logits differ by {err:.3e}")
    assert err <= model_checks.MASK_LOGIT_ATOL
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.forward_selected([frames], text, targets)


def test_native_inference_against_the_reference(golden, dev):
    """Native segment_video / segment_objects against the arrays of the reference's own inference_davis.py:203-261 statements."""
    from ocpg_amd import _lib, inference
    g = golden("infer_collate")
    m = g.meta
    _, model, _ = model_checks.build_product(m, dev)
    frames = g["infer_frames"].to(dev)
    texts = _texts(m, dev)
    origin, clip = tuple(m["origin"]), m["crop_len"]
    calls = _lib.census(True)
    try:
        for obj, text in enumerate(texts):
            logits, masks = inference.segment_video(model, frames, text, clip_len=clip, origin_size=origin, native=True)
            assert logits.shape == g[f"infer_logits{obj}"].shape and masks.shape == g[f"infer_masks{obj}"].shape
            el = (logits.float().cpu() - g[f"infer_logits{obj}"]).abs().max().item()
            em = (masks.cpu() - g[f"infer_masks{obj}"]).abs().max().item()
            assert el <= ATOL_LOGITS and em <= ATOL_MASKS, (obj, el, em)
        assert calls.get("ocpg_mask_tail_f32", 0) == 2                                  # one launch per expression: the whole video
        logits, labels = inference.segment_objects(model, frames, texts, clip_len=clip, origin_size=origin)
        assert calls.get("ocpg_mask_tail_f32", 0) == 2 + 3                              # one merge launch per clip (2 + 2 + 1 frames)
    finally:
        _lib.census(False)
    for obj in range(2):
        assert (logits[obj].float().cpu() - g[f"infer_logits{obj}"]).abs().max().item() <= ATOL_LOGITS
    assert labels.dtype == torch.uint8 and labels.shape == g["infer_labels"].shape
    bad = (labels.cpu() != g["infer_labels"]).float().mean().item()
    assert bad <= LABEL_MISMATCH, bad
