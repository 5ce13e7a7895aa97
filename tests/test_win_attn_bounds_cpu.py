"""The harness of tests/test_win_attn_ref_gpu.py has teeth (tests/win_attn_ref.py, CPU only): a plain-torch emulator with the window
attention kernels' rounding points stays within 0.9 of the derived elementwise bound on every output of every case and dtype, and
each one-line mutant of it (mask -inf instead of -100, bias transposed, last key dropped, region row bw // (BW/NW) instead of
bw % NW) exceeds the bound at least fourfold on the cases it applies to.  With i.i.d. random regions the -inf mutant is NOT seen:
that blind spot of the older tests is why the `blocks` cases plant a masked key that carries weight."""
import pytest
import torch

import win_attn_ref as wr

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
WINDOW = (8, 7, 7)


def _prepared(case, dtype):
    index = wr.swin_index(WINDOW)[:case.n, :case.n]
    return wr.prepared(case, dtype, index, wr.table_rows(WINDOW))


def _emulate(inp, mutant=None):
    return wr.emulate(inp["qkv"], inp["bias"], inp["region"], inp["scale"], inp["nw"], inp["go"], inp["index"],
                      inp["table"].shape[0], mutant)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", wr.CASES, ids=wr.CASE_IDS)
def test_emulator_within_the_bound(case, dtype):
    inp, R, B = _prepared(case, dtype)
    res = wr.ratios(_emulate(inp), R, B)
    print("emulator %s %s: %s" % (case.name, dtype, wr.fmt(res)))
    assert set(res) == set(wr.OUTPUTS) | {"dtable"}
    assert max(res.values()) <= 0.9, res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mutant", wr.MUTANTS)
@pytest.mark.parametrize("case", wr.CASES, ids=wr.CASE_IDS)
def test_mutant_exceeds_the_bound(case, mutant, dtype):
    inp, R, B = _prepared(case, dtype)
    res = wr.ratios(_emulate(inp, mutant), R, B)
    print("%s %s %s: %s" % (mutant, case.name, dtype, wr.fmt(res)))
    if wr.mutant_applies(mutant, case):
        assert max(res.values()) >= 4.0, res
    elif mutant == "neginf" and case.kind == "random":
        # documentation of the blind spot: no masked key carries weight, exp(-100) and exp(-inf) are the same to every output
        assert max(res.values()) <= 0.9, res
        ok = wr.ratios(_emulate(inp), R, B)
        assert all(abs(res[k] - ok[k]) <= 1e-6 * max(ok[k], 1e-30) for k in ok), (res, ok)


def test_cases_cover_what_they_claim():
    names = set(wr.CASE_IDS)
    assert {"blocks-n%d" % n for n in (1, 31, 32, 33, 64, 65, 129)} <= names and len(names) == len(wr.CASES)
    for case in wr.CASES:
        assert case.bw % case.nw == 0
        region = wr.make_regions(case)
        if case.kind == "none":
            assert region is None
            continue
        uniform = [bool((region[w] == region[w, 0]).all()) for w in range(case.nw)]
        if case.kind == "blocks":
            assert uniform[0] and int(region[0, 0]) != 0                  # non-null region, no masked pair: `shifted` is false
            if case.n > 2:
                assert not uniform[1] and int(region[1, 0]) != int(region[1, case.n - 1])
            if case.nw == 4:                                              # only the last token differs
                assert int((region[3] != region[3, 0]).sum()) == 1 and int(region[3, -1]) != int(region[3, 0])
    # the planted key: masked for query 0, and still the heaviest key of that row in the reference
    case = wr.by_name("blocks-n65")
    inp, R, _ = _prepared(case, torch.bfloat16)
    assert wr.has_planted_key(case) and float(R["mask"][1, 0, 0, -1]) == -100.0
    assert float(R["p"][1, :, 0, -1].min()) > 0.999
    # the index helper is the sliced Swin index: linear in a per-token code, inside the table
    idx = wr.swin_index(WINDOW)
    assert idx.shape == (392, 392) and int(idx.min()) == 0 and int(idx.max()) == wr.table_rows(WINDOW) - 1
    a = idx[:, 0] - idx[0, 0]
    assert torch.equal(a[:, None] - a[None, :] + idx[0, 0], idx)
