"""The harness of tests/test_attn_ref_gpu.py has teeth (tests/attn_ref.py, CPU only): a plain-torch emulator with the rounding points of
csrc/attn_smallk.hip / csrc/attn_longk.hip stays within the derived elementwise bound on every output of every case and dtype; each gross
one-line mutant of it (last key ignored, padding row of entry 0 for every entry, last token's dK / dV share lost, second window's dq share
lost, only the last token group of a workgroup summed, lse without the running maximum) exceeds the bound at least fourfold where it
applies; and the two CONTRACT mutants (q * scale, or the probabilities and dS, rounded to the storage type instead of kept in fp32)
exceed it at least fourfold on `out` in bf16.  The older tests' criterion, max|got - ref| <= tol max|ref| + 1e-6 on out / dq / dk / dv,
passes both contract mutants and never reads lse: that blind spot is asserted here too."""
import pytest
import torch

import attn_ref as ar

DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _emulate(inp, kernel, mutant=None):
    return ar.emulate(inp["q"], inp["k"], inp["v"], inp["go"], inp["key_pad"], inp["scale"], inp["h"], inp["keep"], kernel, mutant)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_emulator_within_the_bound(case, dtype):
    inp, R, B = ar.prepared(case, dtype)
    res = ar.ratios(_emulate(inp, case.kernel), R, B)
    print("emulator %s %s: %s" % (case.name, dtype, ar.fmt(res)))
    assert set(res) == set(ar.OUTPUTS)
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", [c for c in ar.CASES if c.kernel == "short" and c.lk in (1, 9, 32) and c.pdrop == 0], ids=lambda c: c.name)
def test_emulator_of_short_keys_on_the_long_key_kernel_within_its_bound(case, dtype):
    """The long-key entry points serve 1-32 keys as a one-chunk window; tests/test_attn_ref_gpu.py runs them there."""
    inp, R, B = ar.prepared(case, dtype, kernel="long")
    res = ar.ratios(_emulate(inp, "long"), R, B)
    print("emulator long %s %s: %s" % (case.name, dtype, ar.fmt(res)))
    assert max(res.values()) <= 1.0, res
    # and as the raw ABI returns dk / dv, in fp32: the bound without the wrapper's rounding term
    B = ar.prepared(case, dtype, kernel="long", abi=True)[2]
    got = ar.emulate(inp["q"], inp["k"], inp["v"], inp["go"], inp["key_pad"], inp["scale"], inp["h"], inp["keep"], "long", abi=True)
    res = ar.ratios(got, R, B)
    print("emulator long ABI %s %s: %s" % (case.name, dtype, ar.fmt(res)))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mutant", ar.GROSS_MUTANTS)
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_gross_mutant_exceeds_the_bound(case, mutant, dtype):
    if not ar.mutant_applies(mutant, case):
        assert ar.why_not(mutant, case)
        return
    inp, R, B = ar.prepared(case, dtype)
    got = _emulate(inp, case.kernel, mutant)
    res = ar.ratios(got, R, B)
    print("%s %s %s: %s" % (mutant, case.name, dtype, ar.fmt(res)))
    assert max(res.values()) >= 4.0, res
    if mutant == "lsemax":
        # only lse moves, and the older tests do not read it: everything they read is bit-equal to the emulator without the mutant, and
        # their criterion holds (one key: dq and dk are exactly 0 in the reference and that criterion an absolute 1e-6 there, so out and dv
        # are held to it)
        plain = _emulate(inp, case.kernel)
        assert res["lse"] >= 4.0 and all(torch.equal(got[k], plain[k]) for k in ("out", "dq", "dk", "dv")), res
        old = ar.old_criterion(got, R, dtype)
        assert max(old[k] for k in (("out", "dv") if case.lk == 1 else ("out", "dq", "dk", "dv"))) < 1.0, old


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("mutant", ar.CONTRACT_MUTANTS)
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_contract_mutant_exceeds_the_bound_and_passes_the_old_criterion(case, mutant, dtype):
    if not ar.mutant_applies(mutant, case):
        assert ar.why_not(mutant, case)
        return
    inp, R, B = ar.prepared(case, dtype)
    got = _emulate(inp, case.kernel, mutant)
    res, old = ar.ratios(got, R, B), ar.old_criterion(got, R, dtype)
    print("%s %s %s: %s | old criterion: %s" % (mutant, case.name, dtype, ar.fmt(res), ar.fmt(old)))
    if dtype == torch.bfloat16:
        assert res["out"] >= 4.0, res
    else:
        # fp16: the storage rounding is 8 times finer, the fp32 terms of the bound are not; both mutants still exceed the bound on out in
        # every case they apply to (q16 2.0-12 times, p16 1.2-6.7 times)
        assert res["out"] > 1.0, res
    assert max(old.values()) < 1.0, old                                         # the blind spot of the max|ref| criterion


def _lds_fwd_short(h, lk):                    # ocpg_attn_smallk_fwd: ((size_t)2 * Lk * H * HS + 32) * sizeof(float), HS = 36
    return (2 * lk * h * 36 + 32) * 4


def _gpb_short(lq, b, h):                     # ocpg_attn_smallk_bwd
    tok_per = 256 // h
    groups = (lq + tok_per - 1) // tok_per
    gpb = 1
    while gpb < 16 and (groups // (2 * gpb)) * b >= 512:
        gpb *= 2
    return groups, gpb


def _gpb_long(lq, b, h):                      # ocpg_attn_longk_bwd
    tok_per = 256 // h
    groups = (lq + tok_per - 1) // tok_per
    return groups, (groups * b + 255) // 256


def test_cases_cover_what_they_claim():
    names = set(ar.CASE_IDS)
    assert len(names) == len(ar.CASES)
    shapes = {(c.kernel, c.lq, c.b, c.h, c.lk) for c in ar.CASES}
    assert {("short", 7, 3, 1, 1), ("short", 33, 2, 8, 8), ("short", 33, 2, 8, 9), ("short", 70, 2, 4, 16), ("short", 70, 2, 4, 17),
            ("short", 40, 2, 8, 28), ("short", 40, 2, 8, 29), ("short", 40, 2, 8, 32), ("short", 300, 3, 2, 20), ("short", 131, 256, 8, 9),
            ("long", 77, 1, 4, 33), ("long", 300, 2, 2, 64), ("long", 70, 2, 8, 65), ("long", 19, 1, 1, 96), ("long", 70, 2, 8, 97),
            ("long", 70, 2, 8, 128), ("long", 259, 29, 8, 65), ("short", 640, 3, 8, 9), ("long", 200, 2, 4, 70)} == shapes
    assert all(c.amp == 3.0 for c in ar.CASES if (c.kernel, c.lk) in (("short", 16), ("short", 17), ("long", 65)) and c.b == 2)
    assert all((c.pdrop == 0.3) == (c.name in ("s-drop", "l-drop")) for c in ar.CASES)
    # the short-key forward's dynamic LDS, below and above the default 64-KiB window
    assert (_lds_fwd_short(8, 28), _lds_fwd_short(8, 29), _lds_fwd_short(8, 32)) == (64640, 66944, 73856)
    assert _lds_fwd_short(8, 28) <= 65536 < _lds_fwd_short(8, 29) < _lds_fwd_short(8, 32)
    assert all(_lds_fwd_short(c.h, c.lk) <= 65536 for c in ar.CASES if c.kernel == "short" and not (c.h == 8 and c.lk >= 29))
    # gpb = 2 with a last workgroup that holds fewer groups than gpb, and a ragged last group
    for name, host in (("s-gpb2", _gpb_short), ("l-gpb2", _gpb_long)):
        c = ar.by_name(name)
        groups, gpb = host(c.lq, c.b, c.h)
        nblocks = (groups + gpb - 1) // gpb
        assert gpb == 2 and groups - (nblocks - 1) * gpb == 1 and c.lq % (256 // c.h) != 0, (name, groups, gpb)
        geo = ar.case_geometry(c)
        assert (geo["groups"], geo["gpb"], geo["nblocks"], geo["last"]) == (groups, 2, nblocks, 1)
    assert (ar.case_geometry(ar.by_name("s-gpb2"))["groups"], ar.case_geometry(ar.by_name("s-gpb2"))["nblocks"]) == (5, 3)
    assert (ar.case_geometry(ar.by_name("l-gpb2"))["groups"], ar.case_geometry(ar.by_name("l-gpb2"))["nblocks"]) == (9, 5)
    for c in ar.CASES:
        host = _gpb_short if c.kernel == "short" else _gpb_long
        assert ar.case_geometry(c)["gpb"] == host(c.lq, c.b, c.h)[1]
        if c.name not in ("s-gpb2", "l-gpb2"):
            assert ar.case_geometry(c)["gpb"] == 1
    # padding: no entry fully padded; the planted key is padded for entry 0 and would carry token 0's weight; entry 1 pads key 0
    padded = [c for c in ar.CASES if c.pad != "none"]
    assert len(padded) >= 14 and all(c.lk > 1 for c in padded)
    for c in padded:
        pad = ar.make_pad(c)
        assert not pad.all(1).any() and bool(pad[0, -1]) and (c.b == 1 or bool(pad[1, 0]))
        inp = ar.make_inputs(c, torch.bfloat16)
        assert torch.equal(inp["k"][-1, 0].float(), 4.0 * inp["q"][0, 0].float())
        s = ar.SCALE * torch.einsum("hd,khd->hk", inp["q"][0, 0].double().view(c.h, 32), inp["k"][:, 0].double().view(c.lk, c.h, 32))
        w = torch.softmax(s, -1)[:, -1]
        assert float(w.min()) > 0.999, (c.name, w)
    c = ar.by_name("l-k64-chunks")
    pad = ar.make_pad(c)
    assert bool(pad[0, :32].all()) and bool(pad[1, 32:].all()) and not bool(pad[0, 32:63].any()) and not bool(pad[1, 1:32].any())
    assert bool(ar.make_pad(ar.by_name("l-k33"))[0, 32])
    # every compile-time key bound of the short-key backward and every window layout of the long-key backward occurs
    lkp = {8 if c.lk <= 8 else 16 if c.lk <= 16 else 32 for c in ar.CASES if c.kernel == "short"}
    assert lkp == {8, 16, 32}
    assert {c.lk for c in ar.CASES if c.kernel == "short"} >= {8, 9, 16, 17}
    layouts = {tuple(n for _, n in ar.case_geometry(c)["windows"]) for c in ar.CASES if c.kernel == "long"}
    layouts |= {tuple(n for _, n in ar.case_geometry(c, "long")["windows"]) for c in ar.CASES if c.kernel == "short" and c.lk in (1, 9, 32)}
    assert layouts == {(1,), (2,), (2, 1), (2, 2)}
    assert {c.lk for c in ar.CASES if c.kernel == "long"} >= {33, 64, 65, 96, 97, 128}
    # a mutant that does not apply says why
    for c in ar.CASES:
        for mutant in ar.MUTANTS:
            assert ar.mutant_applies(mutant, c) == (ar.why_not(mutant, c) is None)
    assert ar.mutant_applies("padrow", ar.by_name("s-k9")) and not ar.mutant_applies("padrow", ar.by_name("l-k33"))
    assert ar.mutant_applies("window2", ar.by_name("l-k65-peaked")) and not ar.mutant_applies("window2", ar.by_name("l-k64-chunks"))
    assert [c.name for c in ar.CASES if ar.mutant_applies("groupsum", c)] == ["s-gpb2", "l-gpb2"]
