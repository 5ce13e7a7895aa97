"""csrc/mask_rle.hip on the MI355X: counts, run numbers and strings of the planes form equal to postprocessors.rle_counts /
rle_encode through the C ABI (into outputs and a workspace pre-filled with 0xFF, guard bytes intact), argument errors, the binding
against the raw entries, the logits form against the float64 referee of tests/mask_tail_ref.py and against ocpg_mask_tail_f32's
bytes, the post-processors' strings on GPU tensors against their host loop, and engine.evaluate_a2d(dump=...) on the fixture model.
tests/test_mask_rle_cpu.py asserts the properties of the seeded inputs."""
import json

import numpy as np
import pytest
import torch

import cases
import mask_rle_cases as M
import mask_tail_ref as R
import model_checks
import refmask_cases as C
from ocpg_amd.models import postprocessors as P
from ocpg_amd.models.ops.functions import mask_rle_func as F

pytestmark = pytest.mark.gpu

LABEL_MISMATCH = 1e-4          # tests/test_mask_tail_gpu.py: the project's bound for decisions of two kernels, as a share of the pixels
GUARD = 24                     # elements around every output


def _guarded(n, dtype, dev):
    """-> (whole buffer of 0xFF bytes, the n elements in its middle)."""
    buf = torch.full(((n + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    b = buf.view(torch.uint8)
    e = buf.element_size()
    return bool((b[:GUARD * e] == 0xFF).all() and (b[(GUARD + n) * e:] == 0xFF).all())


def _finish(n, sizes, max_n, n_trans, ws, dev):
    """Step 2 on what a pack entry left: -> per mask (counts list, string bytes), everything around them checked."""
    from ocpg_amd._lib import lib, stream_ptr
    nt_buf, nt = n_trans
    torch.cuda.synchronize()
    assert _intact(nt_buf, n)
    nt_host = nt.cpu()
    start = torch.zeros(n, dtype=torch.int64)
    start[1:] = torch.cumsum(nt_host[:-1].long() + 1, 0)
    cap = int(start[-1]) + int(nt_host[-1]) + 1
    c_buf, counts = _guarded(cap, torch.int32, dev)
    r_buf, n_runs = _guarded(n, torch.int32, dev)
    b_buf, text = _guarded(7 * cap, torch.uint8, dev)
    l_buf, n_bytes = _guarded(n, torch.int64, dev)
    rc = lib().ocpg_mask_rle_encode(n, max_n, nt_host.data_ptr(), start.data_ptr(), start.to(dev).data_ptr(), cap, counts.data_ptr(),
                                    n_runs.data_ptr(), text.data_ptr(), n_bytes.data_ptr(), ws.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(c_buf, cap) and _intact(r_buf, n) and _intact(b_buf, 7 * cap) and _intact(l_buf, n)
    counts, n_runs, text, n_bytes = counts.cpu(), n_runs.cpu(), text.cpu(), n_bytes.cpu()
    assert torch.equal(n_runs, nt_host + 1)
    out = []
    for m in range(n):
        s, nb = int(start[m]), int(n_bytes[m])
        assert 0 < nb <= 7 * int(n_runs[m])
        assert (text[7 * s + nb:7 * (s + int(n_runs[m]))] == 0xFF).all()                 # nothing written behind a string
        out.append((counts[s:s + int(n_runs[m])].tolist(), text[7 * s:7 * s + nb].numpy().tobytes()))
    return out


def _raw_planes(planes, dev, shifts=None, max_n=None):
    """ocpg_mask_rle_pack_u8 + ocpg_mask_rle_encode on uint8 / bool planes packed into one buffer, plane i starting `shifts[i]` bytes
    behind the previous one's end."""
    from ocpg_amd._lib import lib, stream_ptr
    n = len(planes)
    shifts = shifts or [0] * n
    offs, total = [], 0
    for p, s in zip(planes, shifts):
        total += s
        offs.append(total)
        total += p.numel()
    buf = torch.full((total + 8,), 0x5A, dtype=torch.uint8, device=dev)                  # set bytes in every gap: a read outside a plane shows
    for p, o in zip(planes, offs):
        buf[o:o + p.numel()].view(p.shape).copy_(p.view(torch.uint8) if p.dtype == torch.bool else p)
    sizes = [tuple(p.shape) for p in planes]
    max_n = max_n or max(h * w for h, w in sizes)
    geom = torch.tensor(sizes, dtype=torch.int32)
    off = torch.tensor(offs, dtype=torch.int64).to(dev)
    ws = torch.full((F.workspace_bytes(n, max_n),), 0xFF, dtype=torch.uint8, device=dev)
    n_trans = _guarded(n, torch.int32, dev)
    rc = lib().ocpg_mask_rle_pack_u8(buf.data_ptr(), off.data_ptr(), n, geom.data_ptr(), geom.to(dev).data_ptr(), max_n, n_trans[1].data_ptr(),
                                     ws.data_ptr(), stream_ptr())
    assert rc == 0
    return _finish(n, sizes, max_n, n_trans, ws, dev)


def _expect(plane):
    plane = (plane != 0).numpy()
    return P.rle_counts(plane), P.rle_encode(plane)["counts"]


def test_chunk_size():
    assert F.chunk_pixels() == M.CHUNK and M.CHUNK % 64 == 0


@pytest.mark.parametrize("name", list(M.planes()))
def test_planes_one_by_one(dev, name):
    plane = M.planes()[name]
    (counts, text), = _raw_planes([plane.to(dev)], dev)
    want_counts, want_text = _expect(plane)
    assert counts == want_counts
    assert text == want_text
    # the mask's size in a workspace laid out for a larger one
    (counts, text), = _raw_planes([plane.to(dev)], dev, max_n=plane.numel() + 3 * M.CHUNK + 5)
    assert counts == want_counts and text == want_text


def test_planes_as_a_batch_at_odd_offsets_other_bytes_and_bool(dev):
    planes = M.planes()
    names = list(planes)
    batch = [M.other_bytes(planes[k], seed=i) for i, k in enumerate(names)]             # bytes other than 0 / 1
    shifts = [(1, 3)[i % 2] for i in range(len(batch))]                                  # byte offsets 1 and 3 between differently sized planes
    got = _raw_planes([b.to(dev) for b in batch], dev, shifts=shifts)
    for k, g in zip(names, got):
        assert g == _expect(planes[k]), k
    got = _raw_planes([planes[k].bool().to(dev) for k in names], dev, shifts=shifts[::-1])         # bool storage
    for k, g in zip(names, got):
        assert g == _expect(planes[k]), k


def test_binding_equals_the_host_loop(dev):
    planes = M.planes()
    want = [P.rle_encode(p) for p in planes.values()]
    assert F.rle_encode_masks([p.to(dev) for p in planes.values()]) == want                        # default: the kernels
    assert F.rle_encode_masks([p.bool().to(dev) for p in planes.values()], native=True) == want
    assert F.rle_encode_masks([p.to(dev) for p in planes.values()], native=False) == want
    stack = torch.stack([planes["63x5"][:63], planes["64x5"][:63], planes["65x5"][:63]]).to(dev)
    assert F.rle_encode_masks(stack) == [P.rle_encode(p) for p in stack.cpu()]
    assert F.rle_encode_masks(stack.transpose(1, 2)) == [P.rle_encode(p) for p in stack.transpose(1, 2).cpu()]       # not contiguous
    with pytest.raises(RuntimeError, match="GPU"):
        F.rle_encode_masks([planes["63x5"].to(dev), planes["64x5"]], native=True)


def test_argument_errors_leave_the_outputs_untouched(dev):
    from ocpg_amd._lib import lib, stream_ptr
    L = lib()
    n = 2
    plane = torch.ones(256, dtype=torch.uint8, device=dev)
    geom = torch.tensor([[10, 12], [9, 11]], dtype=torch.int32)
    geom_dev = geom.to(dev)
    off = torch.tensor([0, 120], dtype=torch.int64, device=dev)
    max_n = 120
    q = torch.full((3,), -7, dtype=torch.int64)                                          # host words the query may write
    assert L.ocpg_mask_rle_query(0, 5, q.data_ptr(), q.data_ptr() + 8, None) == -1006 and L.ocpg_mask_rle_query(1, 0, q.data_ptr(), None, None) == -1006
    assert L.ocpg_mask_rle_query(1, 1 << 31, q.data_ptr(), None, None) == -2603 and L.ocpg_mask_rle_query(65536, 9, q.data_ptr(), None, None) == -1008
    assert (q == -7).all() and L.ocpg_mask_rle_query(n, max_n, None, None, None) == 0
    assert F.workspace_bytes(n, max_n) >= n * (64 * 8 + 8 + 4) and F.workspace_bytes(n, max_n) % 8 == 0
    ws = torch.full((F.workspace_bytes(n, max_n) + 8,), 0xFF, dtype=torch.uint8, device=dev)
    n_trans = torch.full((n,), -7, dtype=torch.int32, device=dev)

    def pack(**over):
        a = {"base": plane.data_ptr(), "off": off.data_ptr(), "n_masks": n, "geom_host": geom.data_ptr(), "geom": geom_dev.data_ptr(),
             "max_n": max_n, "n_trans": n_trans.data_ptr(), "workspace": ws.data_ptr()}
        a.update(over)
        return L.ocpg_mask_rle_pack_u8(*a.values(), stream_ptr())

    def g(i, k, v):
        x = geom.clone()
        x[i, k] = v
        return x
    keep = []                                                                            # host tables alive over the calls
    for kw in ({"n_masks": 0}, {"max_n": 0}, {"n_masks": -1}):
        assert pack(**kw) == -1006, kw
    for i, k in ((0, 0), (1, 1)):
        keep.append(g(i, k, 0))
        assert pack(geom_host=keep[-1].data_ptr()) == -1006
    keep.append(torch.tensor([[1 << 16, 1 << 15], [9, 11]], dtype=torch.int32))
    assert pack(geom_host=keep[-1].data_ptr(), max_n=(1 << 31) - 1) == -2603                                     # H * W = 2^31
    assert pack(max_n=1 << 31) == -2603
    assert pack(max_n=119) == -2604                                                      # a mask larger than the stated maximum
    assert pack(geom_host=None) == -2605 and pack(geom=None) == -2605
    keep.append(torch.ones(65536, 2, dtype=torch.int32))
    assert pack(n_masks=65536, geom_host=keep[-1].data_ptr()) == -1008                   # grid axis
    assert pack(n_trans=None) == -1015
    assert pack(workspace=None) == -2606 and pack(workspace=ws.data_ptr() + 4) == -2606
    assert pack(base=None) == -1001 and pack(off=None) == -1001
    torch.cuda.synchronize()
    assert (n_trans == -7).all() and (ws == 0xFF).all()

    # the logits form
    src = torch.zeros(2, 3, 5, 7, device=dev)
    lgeom = torch.tensor([[20, 28, 10, 12], [18, 25, 9, 11]], dtype=torch.int32)
    lgeom_dev = lgeom.to(dev)
    ws6 = torch.full((F.workspace_bytes(6, max_n),), 0xFF, dtype=torch.uint8, device=dev)
    n_trans6 = torch.full((6,), -7, dtype=torch.int32, device=dev)

    def packl(**over):
        a = {"src": src.data_ptr(), "B": 2, "Q": 3, "hs": 5, "ws": 7, "up": 4, "geom_host": lgeom.data_ptr(), "geom": lgeom_dev.data_ptr(),
             "max_n": max_n, "thr": 0.5, "invert": 1, "n_trans": n_trans6.data_ptr(), "workspace": ws6.data_ptr()}
        a.update(over)
        return L.ocpg_mask_rle_pack_logits_f32(*a.values(), stream_ptr())

    def gl(i, k, v):
        x = lgeom.clone()
        x[i, k] = v
        keep.append(x)
        return x.data_ptr()
    for kw in ({"B": 0}, {"Q": 0}, {"hs": 0}, {"ws": 0}, {"up": 0}, {"max_n": 0}):
        assert packl(**kw) == -1006, kw
    for k in range(4):
        assert packl(geom_host=gl(1, k, 0)) == -1006
    assert packl(invert=2) == -2601 and packl(invert=-1) == -2601
    assert packl(geom_host=gl(0, 0, 21)) == -2602 and packl(geom_host=gl(1, 1, 29)) == -2602 and packl(up=1) == -2602
    keep.append(torch.tensor([[20, 28, 1 << 16, 1 << 15], [18, 25, 9, 11]], dtype=torch.int32))
    assert packl(geom_host=keep[-1].data_ptr(), max_n=(1 << 31) - 1) == -2603
    assert packl(max_n=119) == -2604
    assert packl(geom_host=None) == -2605 and packl(geom=None) == -2605
    assert packl(n_trans=None) == -1015 and packl(workspace=None) == -2606 and packl(src=None) == -1001
    torch.cuda.synchronize()
    assert (n_trans6 == -7).all() and (ws6 == 0xFF).all()
    # valid, the same sizes do write: logit 0 -> p = 0.5, not above the threshold; inverted: all set = [0, N]
    assert packl() == 0
    torch.cuda.synchronize()
    assert n_trans6.tolist() == [1] * 6
    assert packl(invert=0) == 0
    torch.cuda.synchronize()
    assert n_trans6.tolist() == [0] * 6

    # step 2
    nt = torch.zeros(6, dtype=torch.int32)
    start = torch.arange(6, dtype=torch.int64)
    start_dev = start.to(dev)
    counts = torch.full((6,), -7, dtype=torch.int32, device=dev)
    n_runs = torch.full((6,), -7, dtype=torch.int32, device=dev)
    text = torch.full((42,), 0xFF, dtype=torch.uint8, device=dev)
    n_bytes = torch.full((6,), -7, dtype=torch.int64, device=dev)

    def enc(**over):
        a = {"n_masks": 6, "max_n": max_n, "n_trans_host": nt.data_ptr(), "run_start_host": start.data_ptr(), "run_start": start_dev.data_ptr(),
             "counts_cap": 6, "counts": counts.data_ptr(), "n_runs": n_runs.data_ptr(), "bytes": text.data_ptr(), "n_bytes": n_bytes.data_ptr(),
             "workspace": ws6.data_ptr()}
        a.update(over)
        return L.ocpg_mask_rle_encode(*a.values(), stream_ptr())
    for kw in ({"n_masks": 0}, {"max_n": 0}, {"counts_cap": 0}):
        assert enc(**kw) == -1006, kw
    assert enc(max_n=1 << 31) == -2603
    for k in ("n_trans_host", "run_start_host", "run_start"):
        assert enc(**{k: None}) == -2605, k
    assert enc(counts_cap=5) == -2607                                                    # a capacity smaller than the totals
    keep.append(torch.tensor([0, 0, 0, 1, 0, 0], dtype=torch.int32))
    assert enc(n_trans_host=keep[-1].data_ptr()) == -2607                                # mask 3 has two runs: it overlaps mask 4's start
    keep.append(torch.tensor([0, 0, 0, -1, 0, 0], dtype=torch.int32))
    assert enc(n_trans_host=keep[-1].data_ptr()) == -2607
    assert enc(workspace=None) == -2606
    for k in ("counts", "n_runs", "bytes", "n_bytes"):
        assert enc(**{k: None}) == -1015, k
    torch.cuda.synchronize()
    assert (counts == -7).all() and (n_runs == -7).all() and (text == 0xFF).all() and (n_bytes == -7).all()
    assert enc() == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [120] * 3 + [99] * 3 and n_runs.tolist() == [1] * 6 and n_bytes.tolist() == [2] * 6
    assert text[:2].cpu().numpy().tobytes() == F.counts_to_string([120])


# ---- the logits form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(M.LOGIT_CASES)))
def test_logits_form_against_the_referee_and_the_mask_tail_kernel(dev, index):
    from ocpg_amd.models.ops.functions.mask_tail_func import mask_binary
    src, up, crop, out, want, decided = M.logit_inputs(index)
    n = src.shape[0]
    pixels = out[0] * out[1]
    open_ = (~decided).flatten(1).sum(1)
    print(f"case {index} up {up}: the referee leaves {open_.tolist()} of {pixels} pixels open")
    assert (open_.double() / pixels <= M.OPEN_CAP).all()
    tail = mask_binary(src.to(dev), up, crop, out, threshold=M.THR, on_value=1).cpu().bool()      # ocpg_mask_tail_f32 mode 1
    for invert in (0, 1):
        # the planes once as one sample's queries, once as one query of n samples
        for shape in ((1, n), (n, 1)):
            rles = F.rle_from_logits(src.to(dev).view(*shape, *src.shape[1:]), up, [crop] * shape[0], [out] * shape[0], threshold=M.THR,
                                     invert=bool(invert), native=True)
            flat = [r for sample in rles for r in sample]
            assert len(rles) == shape[0] and len(flat) == n and all(r["size"] == list(out) for r in flat)
            got = torch.stack([torch.from_numpy(P.rle_decode(r)) for r in flat]).bool()
            ref = ~want if invert else want
            assert torch.equal(got[decided], ref[decided])                               # every pixel the referee decides
            diff = (got != (~tail if invert else tail)).flatten(1).sum(1)
            print(f"case {index} up {up} invert {invert} as {shape}: differences against the mask tail's bytes {diff.tolist()}")
            assert (diff.double() <= LABEL_MISMATCH * pixels).all()
            for r, g in zip(flat, got):
                assert F.rle_area(r) == int(g.sum())


@pytest.mark.parametrize("up", C.UPS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_logits_form_areas_inside_the_count_bounds(dev, name, up):
    """Batches of differently sized samples: each mask's area from its odd runs inside the bounds of |P| that
    tests/test_refmask_counts_gpu.py uses."""
    samples = C.CASES[name][3]
    src = C.source(name, up).to(dev)
    for invert in (False, True):
        lo, hi = C.bounds(name, up, invert)
        rles = F.rle_from_logits(src, up, [s[0] for s in samples], [s[1] for s in samples], threshold=C.THR, invert=invert)
        area = torch.tensor([[F.rle_area(r) for r in sample] for sample in rles])
        print(f"{name} up {up} invert {invert}: {int((hi - lo)[..., 1].sum())} pixels open, areas {area.flatten().tolist()}")
        assert all(r["size"] == list(s[1]) for sample, s in zip(rles, samples) for r in sample)
        assert (lo[..., 1] <= area).all() and (area <= hi[..., 1]).all()
        for (w, d), sample in zip(C.expectation(name, up), rles):
            got = torch.stack([torch.from_numpy(P.rle_decode(r)) for r in sample]).bool()
            assert torch.equal(got[d], (~w if invert else w)[d])


# ---- the post-processors ------------------------------------------------------------------------------------------------------------
def test_post_processors_encode_on_the_device(dev, monkeypatch):
    from ocpg_amd import _lib
    out, orig, size = M.post_outputs()
    out_dev = {k: v.to(dev) for k, v in out.items()}
    want_a = P.A2DSentencesPostProcess(native=False)(out_dev, orig, size)
    want_s = P.PostProcessSegm(native=False)([{}, {}], out_dev, orig, size)

    def never(mask):
        raise AssertionError("a plane went to the host loop")
    monkeypatch.setattr(P, "rle_encode", never)
    calls = _lib.census(True)
    try:
        got_a = P.A2DSentencesPostProcess()(out_dev, orig, size)                         # the default for GPU tensors
        got_s = P.PostProcessSegm(native=True)([{}, {}], out_dev, orig, size)
        assert calls.get("ocpg_mask_rle_pack_u8", 0) == 4 and calls.get("ocpg_mask_rle_encode", 0) == 4      # one per sample and module
    finally:
        _lib.census(False)
    for got, want in ((got_a, want_a), (got_s, want_s)):
        for g, w in zip(got, want):
            assert g["rle_masks"] == w["rle_masks"]                                      # byte for byte
            assert g["masks"].is_cuda and torch.equal(g["masks"], w["masks"])
            if "scores" in w:
                assert torch.equal(g["scores"], w["scores"])
    assert [r["size"] for r in got_a[0]["rle_masks"]] == [[40, 53]] * 5 and [r["size"] for r in got_a[1]["rle_masks"]] == [[37, 71]] * 5


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_a2d_dump_on_the_fixture_model(golden, dev, monkeypatch, tmp_path):
    from ocpg_amd import _lib, engine, metrics
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    from ocpg_amd.util.misc import NestedTensor
    from test_refmask_counts_gpu import _WithText
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

    seen = []
    inner = F.rle_from_logits

    def spy(src, up, crops, out_sizes, **kw):
        out = inner(src, up, crops, out_sizes, **kw)
        seen.append((src.detach().cpu(), up, crops, out_sizes, kw, out))
        return out
    monkeypatch.setattr(F, "rle_from_logits", spy)
    want = engine.evaluate_a2d(net, loader, dev, native=True)
    assert not seen
    path = tmp_path / "predictions.json"
    calls = _lib.census(True)
    try:
        got = engine.evaluate_a2d(net, loader, dev, native=True, dump=str(path))
        assert calls.get("ocpg_mask_rle_pack_logits_f32", 0) == len(loader) == calls.get("ocpg_mask_rle_encode", 0)      # one call per batch
        assert calls.get("ocpg_refmask_counts_f32", 0) == len(loader) and "ocpg_mask_rle_pack_u8" not in calls
    finally:
        _lib.census(False)
    assert got == want and len(seen) == len(loader)
    res = metrics.load_coco_results(str(path))
    assert list(res) == [t[0]["image_id"] for _, t in loader] and len(json.loads(path.read_text())) == sum(len(v) for v in res.values())
    for (src, up, crops, sizes, kw, rles), (_, targets) in zip(seen, loader):
        assert up == 1 and kw["invert"] is True and sizes == [targets[0]["orig_size"].tolist()] and crops == [[h, w]]
        ref, decided = R.binary_decision(R.referee(src[0], 1, tuple(crops[0]), tuple(sizes[0])), kw["threshold"])
        ref = ~ref                                                                       # invert
        lo = (ref & decided).flatten(1).sum(1)
        hi = lo + (~decided).flatten(1).sum(1)
        area = torch.tensor([F.rle_area(r) for r in rles[0]])
        print(f"evaluate_a2d dump on {sizes[0]}: {int((hi - lo).sum())} pixels open, areas {area.tolist()}")
        assert (lo <= area).all() and (area <= hi).all()
        for (score, mask), r in zip(res[targets[0]["image_id"]], rles[0]):
            assert np.array_equal(mask.numpy(), P.rle_decode(r)) and 0.0 <= score <= 1.0
