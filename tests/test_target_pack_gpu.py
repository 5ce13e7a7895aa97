"""csrc/target_pack.hip against the torch composition it replaces (build_target_pack native=True vs native=False on the same device):
torch.equal on every output -- nothing here needs a tolerance -- then the launch count, then the matcher and the criterion with the
switch off and on."""
import pytest
import torch

from test_target_pack_cpu import FULL, ORDINARY, PAST_EDGE, UPPER, WRAP, ZERO_W, make_targets

pytestmark = pytest.mark.gpu

FIELDS = ("gt_s", "gt_m", "region_s", "region_l", "region_ls", "weak_s", "weak_l", "w_s", "w_l", "tboxes", "valid_f", "valid_i", "labels")


def to_dev(targets, dev):
    return [{k: v.to(dev) for k, v in t.items()} for t in targets]


def case_targets(name):
    if name == "ragged":           # 40x72 and 33x96 pad to 64x96; one clip without a valid frame
        return make_targets([(40, 72), (33, 96)], 2, [[ORDINARY, ZERO_W], [WRAP, PAST_EDGE]], zero_valid=1)
    if name == "single_const":     # 32x32, no padding, hi == lo, no labels, the full-image box
        return make_targets([(32, 32)], 1, [[FULL]], heat_kind="const", labels=False)
    if name == "single_outside":   # heat only outside the box
        return make_targets([(32, 32)], 1, [[UPPER]], heat_kind="outside")
    assert name == "chunked"       # 17 clips: the 16-clip chunk and one more; sizes beyond the map for some
    boxes = [ORDINARY, ZERO_W, WRAP, PAST_EDGE, FULL, UPPER]
    shapes = [(33 + (5 * i) % 31, 40 + (7 * i) % 56) for i in range(17)]
    return make_targets(shapes, 2, [[boxes[i % 6], boxes[(i + 3) % 6]] for i in range(17)],
                        sizes=[(h, w) if i % 4 else (2 * h, w + 9) for i, (h, w) in enumerate(shapes)], zero_valid=16)


@pytest.mark.parametrize("ls_hw", [(16, 24), (20, 28)])
@pytest.mark.parametrize("strides", [(1, 2, 2), (2, 4, 2)])
@pytest.mark.parametrize("name", ["ragged", "single_const", "single_outside", "chunked"])
def test_native_equals_composition_bit_for_bit(dev, name, strides, ls_hw):
    from ocpg_amd.models.ops.functions.target_pack_func import build_target_pack
    targets = to_dev(case_targets(name), dev)
    ref = build_target_pack(targets, *strides, ls_hw, native=False)
    got = build_target_pack(targets, *strides, ls_hw, native=True)
    from ocpg_amd import _lib
    calls = _lib.census(True)
    build_target_pack(targets, *strides, ls_hw, native=True)
    _lib.census(False)
    assert calls.get("ocpg_target_pack_f32") == 1, "the kernel did not serve this case"
    for k in FIELDS:
        r, g = getattr(ref, k), getattr(got, k)
        if r is None:
            assert g is None, k
            continue
        assert g.is_contiguous() and g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, g.shape, r.dtype, r.shape)
        assert torch.equal(g, r), f"{k}: {(g != r).sum().item()} of {r.numel()} elements differ"


def test_at_most_three_launches_and_no_copy(dev):
    from torch.profiler import ProfilerActivity, profile
    from ocpg_amd.models.ops.functions.target_pack_func import build_target_pack
    targets = to_dev(case_targets("ragged"), dev)
    build_target_pack(targets, 1, 2, 2, (16, 24), native=True)          # library load, allocator warm-up
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        build_target_pack(targets, 1, 2, 2, (16, 24), native=True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print("device events:", names)
    assert any("tp_pack" in n for n in names), names
    copies = [n for n in names if any(w in n.lower() for w in ("memcpy", "memset", "copy"))]
    assert not copies, copies
    assert len(names) <= 3, names


def _criterion_run(dev, native, monkeypatch):
    """match_stacked, then the criterion, on a fixed random outputs dict: Lr=2, B=2, T=2, q=3, masks 64x96 / 32x48, ls_features 12x32x48."""
    from ocpg_amd.models.criterion import SetCriterion
    from ocpg_amd.models.matcher import HungarianMatcher
    from ocpg_amd.models.ops.functions import target_pack_func
    monkeypatch.setattr(target_pack_func, "NATIVE", native)
    lr, b, t, q = 2, 2, 2, 3
    targets = to_dev(make_targets([(64, 96), (64, 96)], t, [[ORDINARY, UPPER], [PAST_EDGE, FULL]], labels=False), dev)
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(s, generator=g).to(dev)       # noqa: E731
    logits, boxes = rnd(lr, b, t, q, 1), torch.cat([0.3 + 0.4 * torch.rand((lr, b, t, q, 2), generator=g),
                                                     0.1 + 0.4 * torch.rand((lr, b, t, q, 2), generator=g)], -1).to(dev)
    qmasks, pm, pml, lsf = rnd(lr, b, t, q, 32, 48), rnd(lr, b, t, 64, 96), rnd(lr, b, t, 32, 48), rnd(b, t, 12, 32, 48)
    matcher = HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2, cost_mask=2, cost_dice=5, num_classes=1)
    names = ("loss_ce", "loss_bbox", "loss_giou", "loss_proj", "loss_mask", "loss_lst", "loss_proj_low", "loss_mask_low", "loss_lst_low")
    crit = SetCriterion(None, 1, matcher, {k: 1.0 for k in names}, 0.1, ["labels", "boxes", "masks"]).to(dev)
    crit.iter = 50000               # half-way through the warm-up: both the mask and the level-set terms carry weight
    pack = target_pack_func.build_target_pack(targets, crit.mask_out_stride, crit.mask_out_stride_low, matcher.mask_out_stride, (32, 48))
    src = matcher.match_stacked(logits, boxes, qmasks, targets, pack)
    layer = lambda i: {"pred_logits": logits[i], "pred_boxes": boxes[i], "pred_masks": pm[i], "pred_masks_low": pml[i]}   # noqa: E731
    outputs = dict(layer(0), ls_features=lsf, main_matcher_index=matcher.as_indices(src[0]), aux_outputs=[layer(1)],
                   aux_matcher_index=[matcher.as_indices(src[1])], _target_pack=pack)
    from ocpg_amd import _lib
    calls = _lib.census(True)
    losses, *_ = crit(outputs, targets)
    _lib.census(False)
    assert calls.get("ocpg_target_pack_f32", 0) == 0, "the criterion built a pack of its own although the model's was for these targets"
    assert len(losses) == 2 * len(names)
    return src.cpu(), {k: v.detach().double().cpu() for k, v in losses.items()}


def test_matcher_and_criterion_switch_off_and_on(dev, monkeypatch):
    """The matched indices are equal, and no loss moves further between the switch off and on than two runs with the switch off
    differ from each other (measured here; every loss kernel sums in a fixed order, so that spread is expected to be zero)."""
    src_a, off_a = _criterion_run(dev, False, monkeypatch)
    src_b, off_b = _criterion_run(dev, False, monkeypatch)
    src_on, on = _criterion_run(dev, True, monkeypatch)
    assert torch.equal(src_a, src_b) and torch.equal(src_a, src_on)
    for k in off_a:
        spread = (off_a[k] - off_b[k]).abs().item()         # the loss kernels' own run-to-run behaviour: the yardstick
        diff = max((on[k] - off_a[k]).abs().item(), (on[k] - off_b[k]).abs().item())
        print(f"{k}: off-vs-off {spread:.3e}, on-vs-off {diff:.3e}")
        assert diff <= spread, (k, diff, spread)
