"""The run-length encoder's host side (models/ops/functions/mask_rle_func.py), on the CPU: the host paths of rle_encode_masks and
rle_from_logits against postprocessors.rle_encode, the vectorised string helper against a plain loop and hand-derived strings, the
post-processors with native=False against today's code, engine.evaluate_a2d(dump=...) and metrics.load_coco_results on the fixture
model of tests/test_a2d_eval_cpu.py (one process and two gloo ranks), and the properties of the seeded inputs that
tests/test_mask_rle_gpu.py relies on."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import mask_rle_cases as M
import test_a2d_eval_cpu as A
from ocpg_amd import engine, metrics
from ocpg_amd.models import postprocessors as P
from ocpg_amd.models.ops.functions import mask_rle_func as F


# ---- the seeded inputs ---------------------------------------------------------------------------------------------------------------
def test_properties_of_the_planes():
    planes = M.planes()
    counts = {k: P.rle_counts(v.numpy()) for k, v in planes.items()}
    assert counts["1x1-set"] == [0, 1] and counts["1x1-clear"] == [1]
    assert counts["all-clear"] == [63] and counts["all-set"] == [0, 63]
    assert len(counts["checker-from-0"]) == 99 and len(counts["checker-from-1"]) == 100
    assert planes["bernoulli-37x53"].numel() % 64 != 0 and len(counts["bernoulli-37x53"]) > 37 * 53 // 3
    blobs = np.asarray(counts["blobs-300x700"])
    assert planes["blobs-300x700"].numel() > 50 * M.CHUNK and blobs.max() > 1 << 16 and (blobs[3:] - blobs[1:-2] < 0).any()
    edges = np.cumsum(blobs)[:-1]
    assert len(set(edges // M.CHUNK)) > 10                                            # transitions in many chunks
    # transitions exactly on chunk starts / none on them while the run goes on
    on = np.cumsum(counts["chunk-start-transitions"])[:-1]
    assert {M.CHUNK, 2 * M.CHUNK, 3 * M.CHUNK, 3 * M.CHUNK + 1} <= set(on.tolist())
    cont = np.cumsum(counts["chunk-start-continues"])[:-1]
    assert not (set(cont.tolist()) & {M.CHUNK, 2 * M.CHUNK, 3 * M.CHUNK}) and len(cont) == 5
    flat = planes["chunk-start-continues"].numpy().reshape(-1, order="F")
    assert flat[M.CHUNK - 1] == flat[M.CHUNK] == 1 and flat[2 * M.CHUNK - 1] == flat[2 * M.CHUNK] == 0 and flat[3 * M.CHUNK - 1] == flat[3 * M.CHUNK] == 1
    other = M.other_bytes(planes["bernoulli-37x53"])
    assert torch.equal(other != 0, planes["bernoulli-37x53"] != 0) and len(other.unique()) > 50


@pytest.mark.parametrize("index", range(len(M.LOGIT_CASES)))
def test_open_share_of_the_logit_cases(index):
    """A condition of the GPU test, not a measurement: the fp64 referee decides all but 0.5 % of every plane."""
    src, up, crop, out, want, decided = M.logit_inputs(index)
    share = 1 - decided.flatten(1).double().mean(1)
    print(f"case {index} up {up} crop {crop} out {out}: open {(~decided).flatten(1).sum(1).tolist()} of {want[0].numel()} pixels per plane")
    assert share.max().item() <= M.OPEN_CAP
    assert {c[1] for c in M.LOGIT_CASES} == {1, 4}


# ---- the host paths ------------------------------------------------------------------------------------------------------------------
def test_host_path_of_rle_encode_masks():
    planes = M.planes()
    want = [P.rle_encode(p) for p in planes.values()]
    assert F.rle_encode_masks(list(planes.values())) == want
    assert F.rle_encode_masks([p.bool() for p in planes.values()], native=False) == want
    assert F.rle_encode_masks([M.other_bytes(p) for p in planes.values()]) == want
    stack = torch.stack([planes["63x5"][:63], planes["64x5"][:63], planes["65x5"][:63]])
    assert F.rle_encode_masks(stack) == [P.rle_encode(p) for p in stack]
    assert F.rle_encode_masks([]) == []
    for rle, p in zip(want, planes.values()):
        assert np.array_equal(P.rle_decode(rle), p.numpy()) and F.rle_area(rle) == int(p.sum())
    with pytest.raises(RuntimeError, match="GPU"):
        F.rle_encode_masks(list(planes.values()), native=True)
    with pytest.raises(ValueError):
        F.rle_encode_masks([torch.zeros(3, 4)])
    with pytest.raises(ValueError):
        F.rle_encode_masks([torch.zeros(2, 3, 4, dtype=torch.bool)])


@pytest.mark.parametrize("invert", [True, False])
def test_host_path_of_rle_from_logits(invert):
    sizes, origs = [(16, 24), (12, 20), (15, 17)], [(32, 48), (27, 40), (19, 23)]
    masks = A._smooth((3 * 5, 16, 24), 21).view(3, 5, 16, 24)
    post = P.A2DSentencesPostProcess()({"pred_logits": torch.zeros(3, 1, 5, 1), "pred_masks": masks[:, None]}, torch.tensor(origs), torch.tensor(sizes))
    got = F.rle_from_logits(masks, 1, sizes, origs, invert=invert)
    assert len(got) == 3 and all(len(g) == 5 for g in got)
    for g, p in zip(got, post):
        planes = p["masks"][:, 0] if invert else ~p["masks"][:, 0]
        assert g == [P.rle_encode(x) for x in planes]
        if invert:
            assert g == p["rle_masks"]
    assert F.rle_from_logits(masks, 1, torch.tensor(sizes), torch.tensor(origs), invert=invert, native=False) == got
    low = A._smooth((3 * 5, 4, 6), 22).view(3, 5, 4, 6)
    up = low.repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert F.rle_from_logits(low, 4, sizes, origs, invert=invert) == F.rle_from_logits(up, 1, sizes, origs, invert=invert)
    with pytest.raises(RuntimeError, match="GPU"):
        F.rle_from_logits(masks, 1, sizes, origs, native=True)
    with pytest.raises(ValueError):
        F.rle_from_logits(masks, 1, [(17, 24)] * 3, origs)
    with pytest.raises(ValueError):
        F.rle_from_logits(masks, 1, sizes, origs[:2])
    with pytest.raises(ValueError):
        F.rle_from_logits(masks[0], 1, sizes, origs)


# ---- the string helper ---------------------------------------------------------------------------------------------------------------
def _loop_string(counts):
    """The inner loop of postprocessors.rle_encode on a count list."""
    out = bytearray()
    for i, c in enumerate(counts):
        x = c - counts[i - 2] if i > 2 else c
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out)


def test_counts_to_string():
    s = F.counts_to_string
    # hand-derived: 5 payload bits per character, low group first, 0x20 = another follows, + 48
    assert s([0]) == b"0" and s([15]) == b"?" and s([16]) == b"`0" and s([1, 1]) == b"11"
    assert s([7]) == b"7" and s([7, 7]) == b"77" and s([7, 7, 7]) == b"777" and s([7, 7, 7, 7]) == b"7770"     # the i > 2 rule
    assert s([5, 3, 9, 2]) == b"539O"                                                  # 2 - 3 = -1 -> one group of 31
    assert s([0, 5, 3]) == b"053"                                                      # a leading zero-length run
    assert s([]) == b""
    # a positive value needs n characters up to 2^(5n-1) - 1, a negative one down to -2^(5n-1)
    for n in range(1, 8):
        top = (1 << (5 * n - 1)) - 1
        assert len(s([top])) == n and len(s([top + 1])) == n + 1
        assert len(s([0, top + 1, 0, 0])) == 1 + (n + 1) + 1 + n                       # the fourth count: 0 - 2^(5n-1), n characters
        for lst in ([top], [top, 3], [1, top, 2], [0, top + 1 if n < 7 else top, 0, 0], [top, 1, 1, 5, 9]):
            assert s(lst) == _loop_string(lst), lst
            assert F.string_to_counts(s(lst)) == lst
    g = np.random.default_rng(5)
    for _ in range(20):
        lst = (g.integers(0, 4, size=int(g.integers(1, 40))) * g.choice([1, 17, 40000, 3 << 20], size=1)).tolist()
        assert s(lst) == _loop_string(lst) and F.string_to_counts(s(lst)) == lst
    for p in M.planes().values():
        counts = P.rle_counts(p.numpy())
        assert s(counts) == P.rle_encode(p)["counts"] and F.string_to_counts(s(counts)) == counts


# ---- the post-processors -------------------------------------------------------------------------------------------------------------
def test_post_processors_with_native_false_return_what_they_return_today():
    out, orig, size = M.post_outputs()
    for native in (False, None):                                                       # CPU tensors: the default is the host loop too
        got = P.A2DSentencesPostProcess(native=native)(out, orig, size)
        for p, o in zip(got, orig.tolist()):
            assert p["masks"].dtype == torch.bool and tuple(p["masks"].shape) == (5, 1, *o)
            assert p["rle_masks"] == [P.rle_encode(q[0]) for q in p["masks"].cpu()]   # today's expression
        results = P.PostProcessSegm(native=native)([{}, {}], out, orig, size)
        for r, o in zip(results, orig.tolist()):
            assert r["masks"].dtype == torch.uint8 and tuple(r["masks"].shape) == (5, 1, *o)
            assert r["rle_masks"] == [P.rle_encode(x[0]) for x in r["masks"].bool().cpu()]
    with pytest.raises(RuntimeError, match="GPU"):
        P.A2DSentencesPostProcess(native=True)(out, orig, size)
    a = P.build_postprocessors(types.SimpleNamespace(rle_native=False), "a2d")
    assert a.native is False and P.build_postprocessors(types.SimpleNamespace(), "jhmdb").native is None
    s = P.build_postprocessors(types.SimpleNamespace(masks=True, rle_native=True), "refcoco")
    assert s["segm"].native is True


# ---- the dump ------------------------------------------------------------------------------------------------------------------------
def _check_dump(path, want_metrics):
    with open(path) as f:
        raw = json.load(f)
    assert [set(p) for p in raw] == [{"image_id", "category_id", "segmentation", "score"}] * len(raw)
    assert all(p["category_id"] == 1 and isinstance(p["segmentation"]["counts"], str) for p in raw)
    res = metrics.load_coco_results(path)
    acc = metrics.RefMaskAccumulator()
    seen = 0
    for samples, targets in A._loader():
        out = A.Stub()(samples, None, targets)
        post = P.A2DSentencesPostProcess()(out, torch.stack([t["orig_size"] for t in targets]), torch.stack([t["size"] for t in targets]))
        for p, t in zip(post, targets):
            mine = res[t["image_id"]]
            assert len(mine) == A.Q
            for (score, mask), s, m in zip(mine, p["scores"], p["masks"][:, 0]):     # the post-processor's query order
                assert score == s.item() and mask.dtype == torch.uint8 and torch.equal(mask.bool(), m)
            g = t["gt_mask"]
            counts = torch.tensor([[int((m.bool() & g).sum()), int(m.sum()), int(g.sum())] for _, m in mine])
            acc.add([t["image_id"]], torch.tensor([[s for s, _ in mine]]), counts[None])
            seen += 1
    assert seen == len(res) == len(A.SAMPLES) and len(raw) == seen * A.Q
    assert acc.summary() == want_metrics                                               # the same integers through the same composition


def test_evaluate_a2d_dump(tmp_path):
    want = engine.evaluate_a2d(A.Stub(), A._loader(), "cpu")
    path = tmp_path / "predictions.json"
    got = engine.evaluate_a2d(A.Stub(), A._loader(), "cpu", dump=str(path))
    assert got == want and set(got) == A.KEYS
    _check_dump(str(path), want)
    # samples without an image_id are numbered (rank, position): the reader returns the tuple
    bare = [(s, [{k: v for k, v in t.items() if k != "image_id"} for t in ts]) for s, ts in A._loader()]
    engine.evaluate_a2d(A.Stub(), bare, "cpu", dump=str(path))
    assert list(metrics.load_coco_results(str(path))) == [(0, i) for i in range(len(A.SAMPLES))]
    # an empty loader still writes a (loadable, empty) list
    assert engine.evaluate_a2d(A.Stub(), [], "cpu", dump=str(path)) == {} and metrics.load_coco_results(str(path)) == {}


def _rank_worker(rank, world, port, path, q):
    import torch.distributed as dist
    torch.set_num_threads(2)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    batches = A._loader()
    mine = batches[1:] if rank == 0 else []                           # one rank has nothing: it enters the collectives all the same
    q.put((rank, engine.evaluate_a2d(A.Stub(), mine, "cpu", dump=path if rank == 0 else path + ".never")))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_dump_once(tmp_path):
    path = str(tmp_path / "predictions.json")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = A._free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=200) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0] == got[1] == engine.evaluate_a2d(A.Stub(), A._loader()[1:], "cpu")
    assert not os.path.exists(path + ".never")                        # rank 0 alone writes
    res = metrics.load_coco_results(path)
    assert list(res) == [A.SAMPLES[2][0], A.SAMPLES[3][0]] and all(len(v) == A.Q for v in res.values())
