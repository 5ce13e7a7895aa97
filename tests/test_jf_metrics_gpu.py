"""csrc/jf_metrics.hip on the MI355X through the C ABI (ocpg_jf_counts_u8): the six counts per (pair, frame) are integers, so every
comparison with the referee of tests/jf_ref.py (a numpy / scipy restatement of the reference's evaluator) is torch.equal.
"""
import numpy as np
import pytest
import torch

import jf_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _call(gt, res, num_gt, num_res, radius, void_label, all_pairs, counts, t=None, h=None, w=None):
    """The raw entry point on device tensors; sizes can be overridden to provoke argument errors."""
    from ocpg_amd._lib import lib, stream_ptr
    T, H, W = gt.shape
    rc = lib().ocpg_jf_counts_u8(gt.data_ptr(), res.data_ptr(), T if t is None else t, H if h is None else h, W if w is None else w,
                                 num_gt, num_res, radius, -1 if void_label is None else void_label, int(all_pairs), counts.data_ptr(),
                                 stream_ptr())
    torch.cuda.synchronize()
    return rc


def _at_offset(a, off, dev):
    """A device copy of the uint8 array starting `off` bytes into its allocation."""
    buf = torch.zeros(a.size + 8, dtype=torch.uint8, device=dev)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return view


def _run(dev, gt, res, G, Rn, radius, void_label, all_pairs, off=0):
    """-> counts [P, T, 6] on the host, after checking the sentinels on both sides of it."""
    P = Rn * G if all_pairs else G
    n = P * gt.shape[0] * 6
    buf = torch.full((n + 16,), SENTINEL, dtype=torch.int32, device=dev)
    counts = buf[8:8 + n].view(P, gt.shape[0], 6)
    assert _call(_at_offset(gt, off, dev), _at_offset(res, off, dev), G, Rn, radius, void_label, all_pairs, counts) == 0
    assert (buf[:8] == SENTINEL).all() and (buf[8 + n:] == SENTINEL).all()
    return counts.cpu()


@pytest.mark.parametrize("name", list(R.CASES))
def test_counts_equal_the_referee(dev, name):
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs(name)
    want = torch.from_numpy(np.array(R.case_counts(name)))
    for off in (0, 1):
        got = _run(dev, gt, res, G, Rn, radius, void_label, all_pairs, off)
        assert torch.equal(got, want), f"{name} at byte offset {off}: {(got != want).sum().item()} of {want.numel()} counts differ"


@pytest.mark.parametrize("name", ["blobs_2x5x3_r1", "blobs_2x65x129_r3", "corner_pixels"])
def test_all_pairs_with_more_proposals_than_objects(dev, name):
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs(name)
    assert all_pairs and (Rn != G or name == "corner_pixels")
    want = torch.from_numpy(np.array(R.case_counts(name)))
    got = _run(dev, gt, res, G, Rn, radius, void_label, True)
    assert got.shape[0] == Rn * G and torch.equal(got, want)
    if Rn != G:                                             # the diagonal call reads pair (g, g) = all-pairs row g * G + g
        diag = _run(dev, gt, res, G, 0, radius, void_label, False)
        assert torch.equal(diag, want.view(Rn, G, -1, 6)[torch.arange(G), torch.arange(G)])


@pytest.mark.parametrize("name", ["void_stripe", "blobs_3x37x83_r1", "blobs_1x200x300_r4"])
def test_void_label_on_and_off(dev, name):
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs(name)
    assert void_label == 255
    on, off = (torch.from_numpy(np.array(R.case_counts(name, 0, v))) for v in (True, False))
    assert not torch.equal(on, off)                         # the stripe changes the counts, so ignoring it cannot pass
    assert torch.equal(_run(dev, gt, res, G, Rn, radius, 255, all_pairs), on)
    assert torch.equal(_run(dev, gt, res, G, Rn, radius, None, all_pairs), off)


def test_radius_larger_than_the_image(dev):
    for name, radius in (("blobs_2x5x3_r1", 10), ("touch_last_row_col", 64), ("blobs_3x37x83_r3", 40)):
        gt, res, G, Rn, r, void_label, all_pairs = R.case_inputs(name)
        want = torch.from_numpy(R.reference_counts(gt, res, G, Rn, radius, void_label, all_pairs))
        assert torch.equal(_run(dev, gt, res, G, Rn, radius, void_label, all_pairs), want)
        # every boundary pixel is matched as soon as the other map has any
        both = (want[..., 2] > 0) & (want[..., 3] > 0)
        if radius >= max(gt.shape[1:]) * 1.5:
            assert torch.equal(want[..., 4][both], want[..., 2][both]) and torch.equal(want[..., 5][both], want[..., 3][both])


def test_radius_64_is_served_and_65_refused(dev):
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs("blobs_1x200x300_r64")
    assert radius == 64                                                        # the served result itself: test_counts_equal_the_referee
    counts = torch.full((G, 1, 6), SENTINEL, dtype=torch.int32, device=dev)
    assert _call(_at_offset(gt, 0, dev), _at_offset(res, 0, dev), G, Rn, 65, void_label, all_pairs, counts) == -2202
    assert (counts == SENTINEL).all()
    assert _call(_at_offset(gt, 0, dev), _at_offset(res, 0, dev), G, Rn, 64, void_label, all_pairs, counts) == 0
    assert torch.equal(counts.cpu(), torch.from_numpy(np.array(R.case_counts("blobs_1x200x300_r64"))))


def test_argument_errors_leave_counts_untouched(dev):
    from ocpg_amd._lib import lib, stream_ptr
    gt = torch.zeros(2, 5, 7, dtype=torch.uint8, device=dev)
    counts = torch.full((4, 2, 6), SENTINEL, dtype=torch.int32, device=dev)
    good = dict(gt=gt.data_ptr(), res=gt.data_ptr(), T=2, H=5, W=7, G=2, R=2, radius=1, void_label=-1, all_pairs=0, counts=counts.data_ptr())
    for want, kw in ((-1006, dict(T=0)), (-1006, dict(H=0)), (-1006, dict(W=-1)), (-1006, dict(G=0)), (-1006, dict(R=0, all_pairs=1)),
                     (-2201, dict(all_pairs=2)), (-2202, dict(radius=0)), (-2202, dict(radius=65)), (-2203, dict(G=255)),
                     (-2203, dict(R=255, all_pairs=1)), (-2204, dict(void_label=256)), (-2204, dict(void_label=-2)),
                     (-2205, dict(H=1 << 16, W=1 << 15)), (-1008, dict(T=65536)), (-1001, dict(gt=0)), (-1001, dict(res=0)),
                     (-1015, dict(counts=0))):
        a = dict(good, **kw)
        rc = lib().ocpg_jf_counts_u8(a["gt"], a["res"], a["T"], a["H"], a["W"], a["G"], a["R"], a["radius"], a["void_label"], a["all_pairs"],
                                     a["counts"], stream_ptr())
        torch.cuda.synchronize()
        assert rc == want, kw
        assert (counts == SENTINEL).all(), kw
    assert _call(gt, gt, 2, 255, 1, None, 0, counts[:2]) == 0                  # R is ignored without all_pairs
    assert (counts[:2] == 0).all() and (counts[2:] == SENTINEL).all()


def test_two_calls_give_equal_results(dev):
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs("blobs_2x65x129_r18")
    a = _run(dev, gt, res, G, Rn, radius, void_label, all_pairs)
    b = _run(dev, gt, res, G, Rn, radius, void_label, all_pairs)
    assert torch.equal(a, b)


def test_graph_replays_reproduce_the_eager_result(dev):
    """Counts are accumulated with atomics after a zeroing kernel: a replay must start from zero again, not from the last result."""
    from ocpg_amd._lib import lib, stream_ptr
    name = "blobs_2x65x129_r3"
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs(name)
    want = torch.from_numpy(np.array(R.case_counts(name)))
    g, r = _at_offset(gt, 0, dev), _at_offset(res, 0, dev)
    counts = torch.full(tuple(want.shape), SENTINEL, dtype=torch.int32, device=dev)
    T, H, W = gt.shape
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = lib().ocpg_jf_counts_u8(g.data_ptr(), r.data_ptr(), T, H, W, G, Rn, radius, -1 if void_label is None else void_label,
                                     int(all_pairs), counts.data_ptr(), stream_ptr())
    assert rc == 0
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(counts.cpu(), want)
    r.copy_(g)                                              # new input, same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts.cpu(), torch.from_numpy(R.reference_counts(gt, gt, G, Rn, radius, void_label, all_pairs)))


def test_binding_picks_the_kernel_within_its_range_and_the_composition_past_it(dev):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.jf_func import jf_counts
    gt, res, G, Rn, radius, void_label, all_pairs = R.case_inputs("blobs_3x37x83_r3")
    g, r = torch.from_numpy(gt.copy()).to(dev), torch.from_numpy(res.copy()).to(dev)
    for rad, kernel_calls in ((radius, 1), (64, 1), (65, None)):
        want = torch.from_numpy(R.reference_counts(gt, res, G, Rn, rad, void_label, all_pairs))
        calls = _lib.census(True)
        got = jf_counts(g, r, G, Rn, radius=rad, void_label=void_label, all_pairs=all_pairs)
        _lib.census(False)
        assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got.cpu(), want)
        assert calls.get("ocpg_jf_counts_u8") == kernel_calls
    with pytest.raises(RuntimeError, match="invalid argument"):
        jf_counts(g, r, G, Rn, radius=65, void_label=void_label, all_pairs=all_pairs, native=True)


@pytest.mark.parametrize("task", ["unsupervised", "semi-supervised"])
def test_evaluate_davis_on_the_gpu_equals_the_cpu_run(dev, tmp_path, task):
    from ocpg_amd import _lib
    from ocpg_amd.eval_davis import evaluate_davis
    davis, results, seqs = R.write_davis_tree(str(tmp_path), task)
    cpu = evaluate_davis(davis, results, task=task, device="cpu", write_csv=False)
    calls = _lib.census(True)
    gpu = evaluate_davis(davis, results, task=task, device=dev, write_csv=False)
    _lib.census(False)
    assert calls.get("ocpg_jf_counts_u8") == len(seqs)                         # one kernel call per sequence
    assert gpu == cpu
