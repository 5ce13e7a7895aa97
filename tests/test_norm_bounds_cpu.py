"""The harness of tests/test_norm_ref_gpu.py has teeth (tests/norm_ref.py, CPU only): a plain-torch emulator with the rounding points of
csrc/layernorm.hip, csrc/fused_ln.hip (dal_*) and csrc/groupnorm.hip stays within the derived elementwise bound on every output of every
case and dtype; each gross one-line mutant of it (one-pass variance, n - 1, eps outside the root, the last row's dgamma / dbeta share lost,
the second grid-stride sweep skipped, Chan's update without the spread of the tile means, the clamped pixels of a ragged tile counted,
the backward's z without the keep mask, the statistics of the neighbouring group) exceeds the bound at least fourfold where it applies;
the two CONTRACT mutants (mean / rstd, or res + dropout(x), rounded to the 16-bit storage type) exceed it at least fourfold in bf16.
The older tests' criterion, max|got - ref| <= tol max|ref| + atol, passes the one-pass variance and the spread-less update on those
tests' own data and shapes, and FAILS the un-mutated emulator at mean = 1000 sigma: both are asserted here."""
import pytest
import torch

import norm_ref as nr

PAIRS = [(c, dt) for c in nr.CASES for dt in nr.DTYPES[c.op]]
PAIR_IDS = ["%s-%s" % (c.name, nr.dtype_id(dt)) for c, dt in PAIRS]
BF16_PAIRS = [(c, dt) for c, dt in PAIRS if nr.io_dtypes(c.op, dt)[0] == torch.bfloat16]


def _touched(case):
    """The outputs a contract mutant must move past four bounds: rstd always; mean unless the case is one constant row (the mean of a
    bf16-representable constant is that constant, and rounding it changes nothing); y where it is stored in fp32 (dal, gn) -- ln's 16-bit
    y carries a storage rounding of 2^-8 |y|, above the 2^-9 |xhat gamma| that a rounded rstd moves it by.  dx / gx / dgamma follow the
    statistics but sit under their own storage rounding in places; they are printed, not asserted."""
    one_const_row = case.pat == "const" and case.r == 1
    return ("rstd",) + (() if one_const_row else ("mean",)) + (() if case.op == "ln" or one_const_row else ("y",))


@pytest.mark.parametrize("case,dtype", PAIRS, ids=PAIR_IDS)
def test_emulator_within_the_bound(case, dtype):
    inp, R, B = nr.prepared(case, dtype)
    res = nr.ratios(nr.emulate(case.op, inp, dtype), R, B)
    print("emulator %s %s: %s" % (case.name, nr.dtype_id(dtype), nr.fmt(res)))
    assert set(res) == set(nr.OUTPUTS[case.op])
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("mutant", nr.GROSS_MUTANTS)
@pytest.mark.parametrize("case,dtype", PAIRS, ids=PAIR_IDS)
def test_gross_mutant_exceeds_the_bound(case, dtype, mutant):
    if not nr.mutant_applies(mutant, case):
        assert nr.why_not(mutant, case)
        return
    inp, R, B = nr.prepared(case, dtype)
    res = nr.ratios(nr.emulate(case.op, inp, dtype, mutant), R, B)
    print("%s %s %s: %s" % (mutant, case.name, nr.dtype_id(dtype), nr.fmt(res)))
    assert max(res.values()) >= 4.0, res


@pytest.mark.parametrize("mutant", nr.CONTRACT_MUTANTS)
@pytest.mark.parametrize("case,dtype", BF16_PAIRS, ids=["%s-%s" % (c.name, nr.dtype_id(dt)) for c, dt in BF16_PAIRS])
def test_contract_mutant_exceeds_the_bound_in_bf16(case, dtype, mutant):
    if not nr.mutant_applies(mutant, case):
        assert nr.why_not(mutant, case)
        return
    inp, R, B = nr.prepared(case, dtype)
    res = nr.ratios(nr.emulate(case.op, inp, dtype, mutant), R, B)
    print("%s %s %s: %s" % (mutant, case.name, nr.dtype_id(dtype), nr.fmt(res)))
    for name in _touched(case):
        assert res[name] >= 4.0, (name, res)


def test_every_mutant_has_a_case_and_every_exclusion_a_reason():
    for mutant in nr.MUTANTS:
        assert any(nr.mutant_applies(mutant, c) for c in nr.CASES), mutant
        for c in nr.CASES:
            assert nr.mutant_applies(mutant, c) == (nr.why_not(mutant, c) is None)
    assert any(nr.mutant_applies("z16", c) for c, dt in BF16_PAIRS)


@pytest.mark.parametrize("case", nr.OLD_CASES, ids=[c.name for c in nr.OLD_CASES])
def test_old_criterion_passes_the_one_pass_variance_on_its_own_data(case):
    """E[x^2] - mean^2 on the older tests' data: every output they read passes their criterion, in every dtype."""
    for dtype in nr.DTYPES[case.op]:
        inp, R, B = nr.prepared(case, dtype)
        old = nr.old_criterion(nr.emulate(case.op, inp, dtype, "onepass"), R, dtype)
        print("onepass %s %s | old criterion: %s" % (case.name, nr.dtype_id(dtype), nr.fmt(old)))
        assert max(old.values()) < 1.0, old


def test_old_criterion_passes_the_spreadless_update_on_dx_of_a_bf16_map():
    """Chan's update without the spread of the tile means, (2, 256, 50, 33) as test_groupnorm_channels_last_kernel draws it: dx of the
    bf16 map passes 2^-7 max|ref|; the new bound sees it on rstd, y and dx."""
    case = nr.by_name("old-gn-2x256x1650")
    assert nr.tiled(case)
    inp, R, B = nr.prepared(case, torch.bfloat16)
    got = nr.emulate(case.op, inp, torch.bfloat16, "nospread")
    old, res = nr.old_criterion(got, R, torch.bfloat16), nr.ratios(got, R, B)
    print("nospread %s: %s | old criterion: %s" % (case.name, nr.fmt(res), nr.fmt(old)))
    assert old["dx"] < 1.0, old
    assert res["rstd"] >= 4.0 and res["y"] >= 4.0, res


@pytest.mark.parametrize("name", ["ln-c384-r8197-offset", "gn-2x256x60-offset"])
def test_old_criterion_fails_a_correct_kernel_at_mean_1000_sigma(name):
    """fp32 input, mean = 1000 sigma: the un-mutated emulator is outside the older criterion (the rounding of the mean alone is
    ~1e-4 sigma) and inside the derived bound: the older criterion cannot simply be pointed at harder data."""
    case = nr.by_name(name)
    dtype = (torch.float32, torch.float32) if case.op == "ln" else torch.float32
    inp, R, B = nr.prepared(case, dtype)
    got = nr.emulate(case.op, inp, dtype)
    old, res = nr.old_criterion(got, R, dtype), nr.ratios(got, R, B)
    print("emulator %s: %s | old criterion: %s" % (name, nr.fmt(res), nr.fmt(old)))
    assert max(res.values()) <= 1.0, res
    assert max(old.values()) > 1.0, old


def test_cases_cover_what_they_claim():
    assert len(set(nr.CASE_IDS)) == len(nr.CASES)
    ln = [c for c in nr.CASES if c.op == "ln"]
    dal = [c for c in nr.CASES if c.op == "dal"]
    gn = [c for c in nr.CASES if c.op == "gn"]
    assert {c.c for c in ln} == {2, 6, 96, 100, 192, 384, 768, 1024}
    assert {nr.ln_chunk(c.c) for c in ln} == {2, 4, 8, 16} and nr.ln_chunk(100) == 2 and nr.ln_chunk(6) == 2
    assert nr.ln_chunk(3) == 0 and nr.ln_chunk(260) == 0 and nr.ln_chunk(1040) == 0
    assert {(c.c, c.r) for c in ln} >= {(96, 16389), (384, 8197), (1024, 4101)} and {1, 5} <= {c.r for c in ln}
    for c in ln + dal:
        geo = nr.case_geometry(c)
        assert geo["sweeps"] == (2 if c.r > 4000 else 1), c.name
        assert (c.r - geo["cover"] == 5) == (c.r > 4000)                   # a ragged handful of rows in the second sweep
    assert {c.c for c in dal} == {4, 64, 256, 260, 512, 768, 1024, 2048} and {c.r for c in dal} == {1, 5, 4101}
    assert {nr.case_geometry(c)["nch_template"] for c in dal} == {1, 2, 4, 8} and {c.p for c in dal} == {0.0, 0.1}
    assert {(c.n, c.c, c.hw) for c in gn if not nr.tiled(c)} == {(1, 8, 1), (1, 64, 3), (2, 256, 60), (1, 256, 257), (2, 512, 255)}
    assert {(c.n, c.c, c.hw) for c in gn if nr.tiled(c)} == {(2, 256, 1500), (2, 256, 1536), (2, 256, 1537)}
    assert [nr.case_geometry(nr.by_name(n))["ragged"] for n in ("gn-t1500-ramp", "gn-t1536-offset", "gn-t1537-outlier")] == [28, 0, 1]
    for path in ("ln", "dal", "gn", "gn-tiled"):
        pats = {c.pat for c in nr.CASES if nr.path(c) == path}
        assert pats >= {"offset", "const", "rowscale"}, (path, pats)
        assert {c.cl for c in gn if nr.path(c) == path} == {False, True} or not path.startswith("gn")
    assert all("ramp" in {c.pat for c in gn if nr.tiled(c) == t} for t in (False, True))
    assert {c.pat for c in nr.CASES} == {"plain", "offset", "const", "tiny", "outlier", "rowscale", "ramp"}
    # the outlier of the one-pixel ragged tile sits in that pixel; gamma has both signs and exact zeros
    inp = nr.make_inputs(nr.by_name("gn-t1537-outlier"), torch.float32)
    assert float(inp["x"][0, 1536].max()) == 1e4 and float(inp["x"][0, :1536].abs().max()) < 10
    for c in nr.CASES:
        gamma = nr.make_inputs(c, nr.DTYPES[c.op][0])["gamma"] if c.r * c.c < 10000 else None
        if gamma is not None:
            assert bool((gamma == 0).any()) and (c.c < 8 or (bool((gamma > 0).any()) and bool((gamma < 0).any())))
            assert 1e-3 <= float(gamma[gamma != 0].abs().min()) and float(gamma.abs().max()) <= 1e2
