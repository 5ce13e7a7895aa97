"""The mask tail without a GPU: the referee's bound (tests/mask_tail_ref.py) is sound and not vacuous, the inputs of the GPU decision
tests have the properties those tests rely on, and the host logic of the native inference path (OCPG.forward_selected,
segment_video(native=True), segment_objects; CPU tensors run the torch composition) agrees with the path it stands in for and with
the reference's own arrays in infer_collate.npz.  MSDeformAttn has no CPU path: the oracle's test double, as in test_model_cpu.py.
"""
import pytest
import torch
import torch.nn.functional as F

import cases
import mask_tail_ref as R
import model_checks

# tests/test_model_gpu.py:869
ATOL_LOGITS, ATOL_MASKS, LABEL_MISMATCH = 2e-4, 5e-4, 1e-4


@pytest.fixture()
def msda_double(monkeypatch):
    from oracle.msda import MSDAOracleFunction
    import ocpg_amd.models.ops.modules.ms_deform_attn as mod
    monkeypatch.setattr(mod, "MSDeformAttnFunction", MSDAOracleFunction)


def _aten_chain(src, up, crop, out):
    x = src[None]
    if up != 1:
        x = F.interpolate(x, scale_factor=up)
    x = x[:, :, :crop[0], :crop[1]]
    return F.interpolate(x, size=out, mode="bilinear", align_corners=False)[0]


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_aten_fp32_meets_the_bound_and_bf16_inputs_do_not(idx):
    """ATen's own fp32 chain sits inside the bound on every shape of the GPU test (so the bound asks nothing fp32 cannot deliver), and
    the bound is tight enough to see a precision loss: the same chain on logits rounded to bf16 breaks it wherever the logits are
    not constants."""
    shape, up, crop, out, kind = R.CASES[idx]
    src = R.logits(shape, kind, 100 + idx)
    ref = R.referee(src, up, crop, out)
    v = _aten_chain(src, up, crop, out)
    rv = ((v.double() - ref["v"]).abs() / ref["bound_v"]).max().item()
    rp = ((v.sigmoid().double() - ref["p"]).abs() / ref["bound_p"]).max().item()
    print(f"{R.case_id(R.CASES[idx])}: ATen at {rv:.3f} of the logit bound, {rp:.3f} of the probability bound")
    assert rv <= 1.0 and rp <= 1.0
    assert ref["bound_p"].max().item() <= 2e-3                       # rough / saturated planes included
    if kind == "smooth" and shape[1] * shape[2] > 6:
        vb = _aten_chain(src.bfloat16().float(), up, crop, out)
        assert ((vb.sigmoid().double() - ref["p"]).abs() / ref["bound_p"]).max().item() > 10


def test_identity_is_sigmoid():
    shape, up, crop, out, kind = R.CASES[2]
    src = R.logits(shape, kind, 102)
    assert torch.equal(R.referee(src, up, crop, out)["p"], torch.sigmoid(src.double()))


def test_functions_on_cpu_follow_the_referee():
    """mask_probabilities / mask_binary / mask_labels on CPU tensors (the torch composition) against the referee, and the input
    conditions of the GPU decision tests: left-out share <= 0.5 %, every class >= 10 % (binary), every label present."""
    from ocpg_amd.models.ops.functions import mask_tail_func as M
    for case in R.BINARY_CASES:
        shape, up, crop, out, kind = case
        src = R.logits(shape, kind, 100 + R.CASES.index(case))
        ref = R.referee(src, up, crop, out)
        assert ((M.mask_probabilities(src, up, crop, out).double() - ref["p"]).abs() <= ref["bound_p"]).all()
        want, ok = R.binary_decision(ref, 0.5)
        assert 1 - ok.double().mean().item() <= 5e-3
        share = want[ok].double().mean().item()
        assert 0.1 <= share <= 0.9, share
        for on in (1, 255):
            got = M.mask_binary(src, up, crop, out, 0.5, on)
            assert got.dtype == torch.uint8 and torch.equal(got[ok], want[ok].to(torch.uint8) * on)
    for k, shape, up, crop, out, seed in R.LABEL_CASES:
        src = R.label_sources(k, shape, seed)
        want, ok = R.label_decision(R.referee(src, up, crop, out), 0.3, 0.1)
        assert 1 - ok.double().mean().item() <= 5e-3
        assert torch.bincount(want[ok].long(), minlength=k + 1).min().item() > 0
        got = M.mask_labels(src, up, crop, out, 0.3, 0.1)
        assert got.dtype == torch.uint8 and torch.equal(got[ok], want[ok])
    # a tie: objects 2 and 3 are the same map, the lower index wins everywhere
    k, shape, up, crop, out, seed = R.LABEL_CASES[1]
    src = R.label_sources(2, shape, seed)
    src = torch.cat([src, src[1:]], 0)
    want, ok = R.label_decision(R.referee(src, up, crop, out), 0.3, 0.1)
    got = M.mask_labels(src, up, crop, out, 0.3, 0.1)
    assert not (want == 3).any() and not (got == 3).any() and (want == 2)[ok].any()
    assert torch.equal(got[ok], want[ok])


def test_functions_reject_bad_geometry():
    from ocpg_amd.models.ops.functions import mask_tail_func as M
    src = torch.zeros(2, 5, 7)
    with pytest.raises(ValueError):
        M.mask_probabilities(src, 4, (21, 28), (10, 10))              # crop beyond hs * up
    with pytest.raises(ValueError):
        M.mask_binary(src, 4, (20, 28), (10, 10), on_value=256)
    with pytest.raises(ValueError):
        M.mask_labels(torch.zeros(256, 1, 2, 2), 1, (2, 2), (2, 2))


def _texts(meta, device):
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    f, s, pm = cases.tiny_text(1)
    return [PrecomputedText((f * a).to(device), (s * b).to(device), pm.to(device)) for a, b in meta["text_scale"]]


def test_native_inference_matches_the_chain_and_the_reference(golden, msda_double):
    """segment_video(native=True) and segment_objects against segment_video / merge_objects and against the arrays the reference's own
    inference_davis.py:203-261 statements produced (two expressions, 5 frames in clips of 2 + 2 + 1, 160 x 200 -> 320 x 400)."""
    from ocpg_amd import inference
    g = golden("infer_collate")
    m = g.meta
    dev = torch.device("cpu")
    _, model, _ = model_checks.build_product(m, dev)
    frames = g["infer_frames"]
    texts = _texts(m, dev)
    origin, clip = tuple(m["origin"]), m["crop_len"]
    old_masks = []
    for obj, text in enumerate(texts):
        lo, mo = inference.segment_video(model, frames, text, clip_len=clip, origin_size=origin)
        ln, mn = inference.segment_video(model, frames, text, clip_len=clip, origin_size=origin, native=True)
        assert ln.shape == lo.shape and mn.shape == mo.shape and mn.dtype == torch.float32
        for name, other_l, other_m in (("chain", lo, mo), ("reference", g[f"infer_logits{obj}"], g[f"infer_masks{obj}"])):
            el, em = (ln - other_l).abs().max().item(), (mn - other_m).abs().max().item()
            assert el <= ATOL_LOGITS and em <= ATOL_MASKS, (obj, name, el, em)
        old_masks.append(mo)
    logits, labels = inference.segment_objects(model, frames, texts, clip_len=clip, origin_size=origin)
    assert tuple(logits.shape) == (2, m["video_len"], 1) and labels.dtype == torch.uint8 and tuple(labels.shape) == (m["video_len"],) + origin
    for obj in range(2):
        assert (logits[obj] - g[f"infer_logits{obj}"]).abs().max().item() <= ATOL_LOGITS
    for name, other in (("merge_objects", inference.merge_objects(torch.stack(old_masks))), ("reference", g["infer_labels"])):
        bad = (labels != other).float().mean().item()
        assert bad <= LABEL_MISMATCH, (name, bad)
    assert labels.unique().numel() > 1


def test_forward_selected_matches_forward(golden, msda_double):
    """forward_selected against forward followed by nearest x4: pred_masks_low replicated x4 is forward's eval pred_masks, the three
    head outputs are the eval branch's; and it refuses training mode and the per-query (A2D) branch."""
    g = golden("infer_collate")
    m = g.meta
    dev = torch.device("cpu")
    _, model, _ = model_checks.build_product(m, dev)
    model.eval()
    frames = g["infer_frames"][:m["crop_len"]]
    text = _texts(m, dev)[1]
    targets = [{"size": torch.as_tensor([int(frames.shape[-2]), int(frames.shape[-1])])}]
    with torch.no_grad():
        full = model([frames], text, targets)
        sel = model.forward_selected([frames], text, targets)
    assert sel["mask_up"] == 4 and "pred_masks" not in sel
    for k in ("pred_logits", "pred_boxes", "reference_points"):
        assert sel[k].shape == full[k].shape and (sel[k] - full[k]).abs().max().item() <= ATOL_LOGITS, k
    low = sel["pred_masks_low"]
    assert low.dim() == 4 and tuple(low.shape[:2]) == (1, frames.shape[0])
    up = F.interpolate(low, scale_factor=4)[:, :, None]
    assert up.shape == full["pred_masks"].shape
    # mask logits to 4 x the probability tolerance (|d sigmoid| <= |d logit| / 4)
    assert (up - full["pred_masks"]).abs().max().item() <= 4 * ATOL_MASKS
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.forward_selected([frames], text, targets)
    _, a2d, _ = model_checks.build_product(m, dev, dataset_file="a2d")
    a2d.eval()
    with pytest.raises(RuntimeError, match="a2d"):
        a2d.forward_selected([frames], text, targets)


def test_native_writer_produces_the_same_png_layout(tmp_path):
    """write_expression_masks(native=True) with a stand-in model: forward_selected's stride-4 logits go through mask_binary and land
    as 0 / 255 PNGs at the original resolution, as test_datasets_cpu.py checks for the default path."""
    import os

    import numpy as np
    from PIL import Image

    from ocpg_amd import inference
    from test_datasets_cpu import _write_tiny_dataset
    root = str(tmp_path)
    names = _write_tiny_dataset(root)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, clips, captions, targets):
            raise AssertionError("the native writer must not run the all-query forward")

        def forward_selected(self, clips, captions, targets):
            t, _, h, w = clips[0].shape
            assert (h, w) == (360, 480) and targets[0]["size"].tolist() == [360, 480] and not self.training
            low = torch.full((1, t, h // 4, w // 4), -10.0)
            if "zebra" in captions[0].lower():
                low[:, :, : h // 8] = 10.0                                                 # top half
            else:
                low[:, :, :, : w // 16] = 10.0                                             # left quarter
            return {"pred_logits": torch.full((1, t, 1, 1), 3.0), "pred_masks_low": low, "mask_up": 4}

    out = str(tmp_path / "out")
    n = inference.write_expression_masks(Stub(), root, "train", out, videos=["vidA"], native=True)
    assert n == 2 * len(names)
    top = np.asarray(Image.open(os.path.join(out, "Annotations", "vidA", "0", names[3] + ".png")))
    left = np.asarray(Image.open(os.path.join(out, "Annotations", "vidA", "1", names[0] + ".png")))
    assert top.shape == (48, 64) and top.dtype == np.uint8 and set(np.unique(top)) == {0, 255}
    assert top[:23].min() == 255 and top[25:].max() == 0 and left[:, :15].min() == 255 and left[:, 17:].max() == 0
