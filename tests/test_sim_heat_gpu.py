"""ocpg_sim_heat_f32 (csrc/sim_heat.hip) through the raw C ABI against the fp64 referee of tests/weak_ref.py, with the bounds, the
fixture condition and the index equality of tests/test_weak_labels_cpu.py (weak_ref.check_head).  Every output sits between sentinel
guards; every case runs once more with the feature pointer at a 16-byte-aligned, non-zero offset into its allocation."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import weak_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7777


def _guarded(n, dtype, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _raw(dev, feat_np, obj_frame, cand_off, cand_xy, box, feat_offset=0, c_override=None, off_host=None):
    """One call of the entry point -> (rc, (heat buffer, view), (choice ...), (score ...))."""
    from ocpg_amd import _lib
    f, h, w, c = feat_np.shape
    store = torch.zeros((feat_np.size + feat_offset,), dtype=torch.float32, device=dev)
    feat = store[feat_offset:]
    feat.copy_(torch.from_numpy(feat_np).reshape(-1))
    assert feat.data_ptr() % 16 == 0 and (feat_offset == 0 or feat.data_ptr() != store.data_ptr())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    n_obj, total = len(obj_frame), int(cand_off[-1])
    host = np.ascontiguousarray(cand_off if off_host is None else off_host, dtype=np.int32)
    d_frame, d_off, d_xy = i32(obj_frame), i32(cand_off), i32(np.asarray(cand_xy).reshape(-1, 2))
    d_box = None if box is None else i32(box)
    heat, choice, score = _guarded(n_obj * h * w, torch.float32, dev), _guarded(n_obj, torch.int32, dev), _guarded(total, torch.float32, dev)
    L = _lib.lib()
    work = torch.empty((int(L.ocpg_sim_heat_workspace(f, h, w, total)) // 4 + 4,), dtype=torch.float32, device=dev)
    rc = L.ocpg_sim_heat_f32(feat.data_ptr(), f, h, w, c if c_override is None else c_override, n_obj, d_frame.data_ptr(),
                             host.ctypes.data_as(ctypes.c_void_p), d_off.data_ptr(), d_xy.data_ptr(),
                             None if d_box is None else d_box.data_ptr(), heat[1].data_ptr(), choice[1].data_ptr(), score[1].data_ptr(),
                             work.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, heat, choice, score


@pytest.mark.parametrize("feat_offset", [0, 12])
@pytest.mark.parametrize("name", list(R.HEAD_CASES))
def test_kernel_within_fp32_bounds_of_the_fp64_referee(dev, name, feat_offset):
    case, _ = R.head_case(name)
    n_obj, total = len(case["obj_frame"]), int(case["cand_off"][-1])
    h, w = case["feat"].shape[1:3]
    rc, heat, choice, score = _raw(dev, case["feat"], case["obj_frame"], case["cand_off"], case["cand_xy"], case["box"], feat_offset)
    assert rc == 0
    for (buf, view), n in ((heat, n_obj * h * w), (choice, n_obj), (score, total)):
        assert _guards_intact(buf, n), name
        assert not bool((view == SENTINEL).any()), name                      # every element written
    R.check_head(name, heat[1].view(n_obj, h, w).cpu().numpy(), choice[1].cpu().numpy(), score[1].cpu().numpy())


def test_kernel_runs_without_a_score_output(dev):
    """score NULL: the scores stay in the workspace, choice and plane are the same."""
    from ocpg_amd import _lib
    name = "23x40x256_multi"
    case, _ = R.head_case(name)
    feat, obj_frame, off, xy, box = (t.contiguous() if t is not None else None for t in R.head_inputs(name, dev))
    f, h, w, c = feat.shape
    n_obj, total = obj_frame.numel(), int(off[-1])
    heat = torch.empty((n_obj, h, w), dtype=torch.float32, device=dev)
    choice = torch.empty((n_obj,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    work = torch.empty((int(L.ocpg_sim_heat_workspace(f, h, w, total)) // 4 + 4,), dtype=torch.float32, device=dev)
    host = np.ascontiguousarray(case["cand_off"], dtype=np.int32)
    rc = L.ocpg_sim_heat_f32(feat.data_ptr(), f, h, w, c, n_obj, obj_frame.data_ptr(), host.ctypes.data_as(ctypes.c_void_p), off.data_ptr(),
                             xy.data_ptr(), box.data_ptr(), heat.data_ptr(), choice.data_ptr(), None, work.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    _, ref = R.head_case(name)
    R.check_head(name, heat.cpu().numpy(), choice.cpu().numpy(), ref["score"].astype(np.float32))


def test_argument_errors_leave_the_outputs_alone(dev):
    case, _ = R.head_case("2x3x8_two")
    args = (case["feat"], case["obj_frame"], case["cand_off"], case["cand_xy"], case["box"])

    def untouched(res):
        return all(bool((buf == SENTINEL).all()) for buf, _ in res[1:])

    res = _raw(dev, *args, c_override=6)                                                      # C % 4 != 0
    assert res[0] == -1005 and untouched(res)
    many = np.array([0, 257], dtype=np.int32)                                                 # more than 256 candidates
    res = _raw(dev, case["feat"], case["obj_frame"], many, np.zeros((257, 2), dtype=np.int32), case["box"])
    assert res[0] == -1008 and untouched(res)
    two = (case["feat"], np.array([0, 0], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), case["cand_xy"],
           np.array([[0, 0, 2, 2]] * 2, dtype=np.int32))
    res = _raw(dev, *two, off_host=np.array([0, 2, 1], dtype=np.int32))                       # cand_off not ascending
    assert res[0] == -1008 and untouched(res)
    res = _raw(dev, *two, off_host=np.array([1, 1, 2], dtype=np.int32))                       # ... or not starting at 0
    assert res[0] == -1008 and untouched(res)
    with pytest.raises(RuntimeError, match="served range"):                                   # the wrapper: the kernel or an error
        from ocpg_amd.models.ops.functions.sim_heat_func import sim_heat
        sim_heat(torch.ones(1, 2, 3, 6, device=dev), torch.zeros(1, dtype=torch.int32), torch.tensor([0, 1]),
                 torch.zeros(1, 2, dtype=torch.int32), None, native=True)


class _PooledBody(nn.Module):
    """A stride-32 stand-in for the ResNet body that needs no convolution library: three stride-32 views of the frame through one
    seeded linear map, made positive like the head fixtures (|.| + 0.05)."""

    def __init__(self, channels, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("weight", torch.randn(channels, 9, generator=g))

    def forward(self, x):
        v = torch.cat([F.avg_pool2d(x, 32), x[:, :, ::32, ::32], x[:, :, 16::32, 16::32]], dim=1)
        return {"0": torch.einsum("fchw,dc->fdhw", v, self.weight).abs() + 0.05}


def test_label_frames_kernel_agrees_with_composition(dev):
    """label_frames at a 23 x 40 x 256 map with the kernel (native=True, and native=None: the GPU default) and with the composition
    (native=False): all are held to the referee's bounds on the same features -- the plane of a candidate whose fp64 score is within
    twice the score bound of the best (with near-equal scores either path may pick either) -- and the call census shows which runs
    the kernel served."""
    from ocpg_amd import _lib
    from ocpg_amd.weak_labels import SimilarityLabeler, mask_centers_and_boxes
    fh, fw = 23 * 32, 40 * 32
    g = torch.Generator().manual_seed(2)
    frames = torch.randn(2, 3, fh, fw, generator=g).to(dev)
    masks = torch.zeros(2, 2, fh, fw, dtype=torch.bool, device=dev)
    masks[0, 0, 100:600, 200:1100] = True                      # 16 x 29 cells: the stride grows
    masks[1, 0, 300:420, 640:700] = True
    masks[1, 1, 0:fh, 0:500] = True
    centers, boxes, valid = mask_centers_and_boxes(masks.flatten(0, 1))
    centers, boxes, valid = centers.view(2, 2, 2).cpu(), boxes.view(2, 2, 4).cpu(), valid.view(2, 2).cpu()
    out = {}
    for native in (True, False, None):
        lab = SimilarityLabeler("resnet50", frames_per_pass=2, native=native)
        lab.body = _PooledBody(256)
        lab = lab.to(dev)
        calls = _lib.census(True)
        out[native] = [t.cpu().numpy() for t in lab.label_frames(frames, centers, boxes, valid)]
        _lib.census(False)
        assert calls.get("ocpg_sim_heat_f32", 0) == (0 if native is False else 2)
    feat = lab.features(frames).cpu().numpy()
    h, w = feat.shape[1:3]
    assert (h, w, feat.shape[3]) == (23, 40, 256)
    for f, o in ((0, 0), (1, 0), (1, 1)):
        cell = R.point_cell(centers[f, o].tolist(), (fh, fw), (h, w))
        pref = R.sim_head(feat, [f], [0, 1], [cell])
        cur, cells = R.box_candidates(boxes[f, o].tolist(), (fh, fw), (h, w))
        bref = R.sim_head(feat, [f], [0, len(cells)], cells, [cur])
        near_best = np.nonzero(bref["score"] >= bref["score"].max() - 2 * bref["score_bound"].max())[0]
        for native in (True, False, None):
            hp, hb = out[native]
            assert (np.abs(hp[f, o].reshape(-1) - pref["s"][0]) <= pref["s_bound"][0]).all(), (native, f, o)
            assert any((np.abs(hb[f, o].reshape(-1) - bref["s"][c]) <= bref["s_bound"][c]).all() for c in near_best), (native, f, o)
    for native in (True, False, None):
        assert not out[native][0][0, 1].any() and not out[native][1][0, 1].any()              # the invisible object
