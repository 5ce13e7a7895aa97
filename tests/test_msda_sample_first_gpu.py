"""Sample-first MSDeformAttn cross-attention (csrc/msda_sample_first.hip) against fp64.

The reference is the library's own fp64 op on value = masked_fill(src . Wv^T + bv, pad, 0) built in fp64 through autograd.  Today's fp32
path (F.linear + masked_fill + MSDeformAttnFunction) runs on the same inputs; a tensor of the new path may be at most
max(4 x today's distance from the fp64 reference, 2e-6) away from it, max-norm relative.  (The two fp32 summation orders sat 1.4e-7 .. 4.8e-7
from each other in a CPU rehearsal of the identity; 2e-6 is four times the worst of those.)"""
import ctypes
import importlib
import warnings

import pytest
import torch
import torch.nn.functional as F

import cases
import module_checks as mc

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
NAMES = ("out", "grad_src", "grad_wv", "grad_bv", "grad_loc", "grad_attn")


def _mda():
    return importlib.import_module("ocpg_amd.models.ops.modules.ms_deform_attn")


def _inputs(N, Lq, M, D, shapes, P, pad_frac=0.0, bias=True, lo=-0.15, hi=1.15, same_loc=None, seed=0):
    g = torch.Generator().manual_seed(1234 + seed)
    C, L = M * D, len(shapes)
    sh, lsi = cases.level_start(shapes)
    S = int(sh.prod(1).sum())
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * (hi - lo) + lo
    if same_loc is not None:
        loc = torch.tensor(same_loc).expand(N, Lq, M, L, P, 2).contiguous()
    d = dict(src=torch.randn(N, S, C, generator=g), wv=torch.randn(C, C, generator=g) / C ** 0.5,
             bv=torch.randn(C, generator=g) * 0.5 if bias else None,
             pad=(torch.rand(N, S, generator=g) < pad_frac) if pad_frac > 0 else None,
             loc=loc, attn=torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P),
             go=torch.randn(N, Lq, C, generator=g), shapes=sh, lsi=lsi, dims=(N, S, M, D, L, Lq, P))
    return d


def _old_order(d, dev, dtype):
    """value_proj -> masked_fill -> the op, in `dtype` (fp64: the reference; fp32: today's path); also grad_value for the untouched-row check"""
    from ocpg_amd.models.ops.functions import MSDeformAttnFunction
    N, S, M, D, L, Lq, P = d["dims"]
    leaf = {k: d[k].to(dev, dtype).requires_grad_(True) for k in ("src", "wv", "loc", "attn")}
    bv = d["bv"].to(dev, dtype).requires_grad_(True) if d["bv"] is not None else None
    value = F.linear(leaf["src"], leaf["wv"], bv)
    if d["pad"] is not None:
        value = value.masked_fill(d["pad"].to(dev)[..., None], 0.0)
    value = value.view(N, S, M, D)
    value.retain_grad()
    out = MSDeformAttnFunction.apply(value, d["shapes"].to(dev), d["lsi"].to(dev), leaf["loc"], leaf["attn"], 64)
    (out * d["go"].to(dev, dtype)).sum().backward()
    r = dict(out=out.detach(), grad_src=leaf["src"].grad, grad_wv=leaf["wv"].grad, grad_bv=None if bv is None else bv.grad,
             grad_loc=leaf["loc"].grad, grad_attn=leaf["attn"].grad, grad_value=value.grad)
    return r


def _new_order(d, dev, keep_forward=False):
    """keep_forward: the function whose forward stays value_proj + op and whose backward alone is the sample-first one"""
    from ocpg_amd.models.ops.functions import ms_deform_attn_func as ff
    SF = ff.MSDeformAttnSampleFirstBackwardFunction if keep_forward else ff.MSDeformAttnSampleFirstFunction
    leaf = {k: d[k].to(dev).requires_grad_(True) for k in ("src", "wv", "loc", "attn")}
    bv = d["bv"].to(dev).requires_grad_(True) if d["bv"] is not None else None
    assert SF.supported(leaf["src"], leaf["wv"], bv, leaf["loc"], leaf["attn"])
    out = SF.apply(leaf["src"], leaf["wv"], bv, None if d["pad"] is None else d["pad"].to(dev), d["shapes"].to(dev), d["lsi"].to(dev),
                   leaf["loc"], leaf["attn"])
    (out * d["go"].to(dev)).sum().backward()
    return dict(out=out.detach(), grad_src=leaf["src"].grad, grad_wv=leaf["wv"].grad, grad_bv=None if bv is None else bv.grad,
                grad_loc=leaf["loc"].grad, grad_attn=leaf["attn"].grad)


def _dist(a, ref):
    scale = ref.abs().max().item()
    err = (a.double() - ref).abs().max().item()
    return err / scale if scale > 0 else err


def _compare(d, dev, tag):
    ref, old, new = _old_order(d, dev, torch.float64), _old_order(d, dev, torch.float32), _new_order(d, dev)
    bad = []
    for k in NAMES:
        if ref[k] is None:
            assert new[k] is None
            continue
        e_old, e_new = _dist(old[k], ref[k]), _dist(new[k], ref[k])
        bound = max(4 * e_old, FLOOR)
        print(f"{tag:12s} {k:10s} today {e_old:.3e}  sample-first {e_new:.3e}  bound {bound:.3e}")
        if not e_new <= bound:
            bad.append((k, e_new, bound))
    assert not bad, bad
    return ref, old, new


CASE1 = dict(N=2, Lq=5, M=8, D=32, shapes=[(12, 20), (6, 10), (3, 5), (2, 3)], P=4, pad_frac=0.15)


def test_padded_four_levels_vs_fp64(dev):
    ref, _, new = _compare(_inputs(**CASE1), dev, "case1")
    # rows of grad_src no sample touches (no gradient reaches value there) stay exactly 0
    untouched = (ref["grad_value"].flatten(2) == 0).all(-1)
    assert untouched.any() and (new["grad_src"][untouched] == 0).all()


def test_single_query_no_mask_no_bias_vs_fp64(dev):
    _compare(_inputs(N=1, Lq=1, M=2, D=32, shapes=[(5, 7), (3, 4)], P=1, bias=False, seed=1), dev, "case2")


def test_all_atomics_collide_vs_fp64(dev):
    """every query and head samples the SAME location: the whole scatter lands on four pixels per level"""
    _compare(_inputs(N=3, Lq=7, M=8, D=32, shapes=[(8, 12), (4, 6), (2, 3)], P=4, same_loc=[0.37, 0.61], seed=2), dev, "case3")


def test_query_outside_the_map(dev):
    """a query whose samples all lie outside every level: its out row is exactly 0 (the bias does not leak) and its grad_loc / grad_attn
    are the reference's (zero)"""
    d = _inputs(**CASE1, seed=3)
    d["loc"][0, 2] = 1.5
    d["loc"][1, 4] = -0.7
    ref, _, new = _compare(d, dev, "case4")
    for n, q in ((0, 2), (1, 4)):
        assert (new["out"][n, q] == 0).all()
        assert (ref["grad_loc"][n, q] == 0).all() and (ref["grad_attn"][n, q] == 0).all()
        assert (new["grad_loc"][n, q] == 0).all() and (new["grad_attn"][n, q] == 0).all()


@pytest.mark.parametrize("case", [CASE1, dict(N=1, Lq=1, M=2, D=32, shapes=[(5, 7), (3, 4)], P=1, bias=False, seed=1)], ids=["case1", "case2"])
def test_forward_keeping_function(dev, case):
    """MSDeformAttnSampleFirstBackwardFunction: `out` has the bits of value_proj + masked_fill + op, the five gradients are the sample-first
    backward's (same bound against fp64 as above) and equal to MSDeformAttnSampleFirstFunction's wherever the summation order is fixed"""
    d = _inputs(**case)
    from ocpg_amd.models.amp_cache import linear
    from ocpg_amd.models.ops.functions import MSDeformAttnFunction
    ref, old, new = _old_order(d, dev, torch.float64), _old_order(d, dev, torch.float32), _new_order(d, dev, keep_forward=True)
    N, S, M, D, L, Lq, P = d["dims"]
    # the module's own value path (its Linear routing picks the GEMM by size), no gradients wanted from it
    value = linear(d["src"].to(dev), d["wv"].to(dev).requires_grad_(True), None if d["bv"] is None else d["bv"].to(dev)).detach()
    if d["pad"] is not None:
        value = value.masked_fill(d["pad"].to(dev)[..., None], 0.0)
    today = MSDeformAttnFunction.apply(value.view(N, S, M, D), d["shapes"].to(dev), d["lsi"].to(dev), d["loc"].to(dev), d["attn"].to(dev), 64)
    assert torch.equal(new["out"], today)
    full = _new_order(d, dev)
    for k in NAMES[1:]:
        if ref[k] is None:
            assert new[k] is None
            continue
        e_old, e_new = _dist(old[k], ref[k]), _dist(new[k], ref[k])
        bound = max(4 * e_old, FLOOR)
        print(f"keep-forward {k:10s} today {e_old:.3e}  sample-first backward {e_new:.3e}  bound {bound:.3e}")
        assert e_new <= bound, (k, e_new, bound)
        if k != "grad_src":
            assert torch.equal(new[k], full[k]), k


def test_default_keeps_the_forward_bits_at_a_size_the_rule_takes(dev, monkeypatch):
    """N * S = 10 200 rows (the model's four levels at 384 x 640, two frames), five queries: by default the rule takes the call, the
    module's three results are bit for bit those of the switch set to 0, and the backward runs the sample-first kernels"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import MSDeformAttn
    m = _mda()
    shapes = [(48, 80), (24, 40), (12, 20), (6, 10)]
    N, Lq, M, D, P, L = 2, 5, 8, 32, 4, 4
    C = M * D
    sh, lsi = cases.level_start(shapes)
    S = int(sh.prod(1).sum())
    assert m.sample_first_wanted(N, S, M, Lq, L, P) and not m.SAMPLE_FIRST_FWD
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(0)
    mod = MSDeformAttn(C, L, M, P).to(dev)
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.02)
        mod.attention_weights.weight.normal_(0, 0.1)
        mod.value_proj.bias.normal_(0, 0.5)
    shd, lsd = sh.to(dev), lsi.to(dev)
    shd._ocpg_host = sh
    pad = (torch.rand(N, S, generator=g) < 0.1).to(dev)
    ref_pts = torch.rand(N, Lq, L, 2, generator=g).to(dev)
    go = torch.randn(N, Lq, C, generator=g).to(dev)
    src = torch.randn(N, S, C, generator=g).to(dev).requires_grad_(True)
    query = torch.randn(N, Lq, C, generator=g).to(dev).requires_grad_(True)
    params = [mod.value_proj.weight, mod.value_proj.bias, mod.sampling_offsets.weight, mod.attention_weights.weight]

    def run(mode):
        monkeypatch.setattr(m, "SAMPLE_FIRST", mode)
        calls = _lib.census(True)
        try:
            out, loc, attn = mod(query, ref_pts, src, shd, lsd, pad)
            grads = torch.autograd.grad((out * go).sum(), [src, query] + params)
        finally:
            _lib.census(False)
        return (out.detach(), loc.detach(), attn.detach()), grads, dict(calls)

    res0, g0, c0 = run("0")
    res1, g1, c1 = run("1")
    assert not any(k.startswith("ocpg_msda_sf_") for k in c0), c0
    assert c1.get("ocpg_msda_sf_bwd_f32", 0) == 1 and c1.get("ocpg_msda_sf_bwd_params_f32", 0) == 1 and "ocpg_msda_bwd_f32" not in c1, c1
    for a, b in zip(res0, res1):
        assert torch.equal(a, b)
    # gradients: two fp32 summation orders of the same sums (and float atomics in grad_src on both sides).  At op level each order may be
    # FLOOR from fp64, so 2 x FLOOR from the other; the query and parameter gradients pass through one more small GEMM each way: 4 x FLOOR
    for k, a, b in zip(("src", "query", "wv", "bv", "offsets_w", "attn_w"), g0, g1):
        e = _dist(b, a.double())
        print(f"default vs 0: grad {k:10s} {e:.3e}")
        assert e <= 4 * FLOOR, (k, e)


def _raw_call(d, dev, fill):
    """the three entry points on caller-owned buffers pre-filled with `fill`"""
    from ocpg_amd._lib import lib, stream_ptr
    N, S, M, D, L, Lq, P = d["dims"]
    C = M * D
    t = {k: d[k].to(dev).contiguous() for k in ("src", "wv", "loc", "attn", "go")}
    bv = d["bv"].to(dev) if d["bv"] is not None else None
    pad = d["pad"].to(dev).view(torch.uint8) if d["pad"] is not None else None
    sh, lsi = d["shapes"].to(dev), d["lsi"].to(dev)
    new = lambda *s: torch.full(s, fill, device=dev)      # noqa: E731
    out, s, beta = new(N, Lq, C), new(N, Lq, M, C), new(N, Lq, M)
    gsrc, gloc, gattn, gwv, gbv = torch.zeros(N, S, C, device=dev), new(N, Lq, M, L, P, 2), new(N, Lq, M, L, P), new(C, C), new(C)
    p = lambda x: None if x is None else x.data_ptr()     # noqa: E731
    rc = [lib().ocpg_msda_sf_fwd_f32(p(t["src"]), p(t["wv"]), p(bv), p(pad), p(sh), p(lsi), p(t["loc"]), p(t["attn"]), N, S, M, D, L, Lq, P,
                                     p(out), p(s), p(beta), stream_ptr()),
          lib().ocpg_msda_sf_bwd_f32(p(t["src"]), p(t["wv"]), p(bv), p(pad), p(sh), p(lsi), p(t["loc"]), p(t["attn"]), p(t["go"]), N, S, M, D, L,
                                     Lq, P, p(gsrc), p(gloc), p(gattn), stream_ptr()),
          lib().ocpg_msda_sf_bwd_params_f32(p(t["go"]), p(s), p(beta), N, M, D, Lq, p(gwv), p(gbv), stream_ptr())]
    torch.cuda.synchronize()
    return rc, dict(out=out, s=s, beta=beta, grad_src=gsrc, grad_loc=gloc, grad_attn=gattn, grad_wv=gwv, grad_bv=gbv)


def test_outputs_are_fully_overwritten(dev):
    d = _inputs(**CASE1, seed=3)
    d["loc"][0, 2] = 1.5                         # skipped samples must be written too
    rc, got = _raw_call(d, dev, float("nan"))
    assert rc == [0, 0, 0]
    for k in ("out", "s", "beta", "grad_loc", "grad_attn", "grad_wv", "grad_bv", "grad_src"):
        assert not torch.isnan(got[k]).any(), k
    new = _new_order(d, dev)
    for k in NAMES:
        if k != "grad_src":
            assert torch.equal(got[k], new[k]), k


@pytest.mark.parametrize("M,D", [(8, 30), (3, 32)])
def test_unserved_shapes_decline_and_the_module_falls_back(dev, M, D, monkeypatch):
    """D = 30 (C = 240) and C = 96: -2000 from every entry point with nothing written; the module keeps value_proj + the generic op"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import MSDeformAttn
    d = _inputs(N=1, Lq=3, M=M, D=D, shapes=[(5, 7), (3, 4)], P=2)
    rc, got = _raw_call(d, dev, 7.0)
    assert rc == [-2000, -2000, -2000]
    for k in ("out", "s", "beta", "grad_loc", "grad_attn", "grad_wv", "grad_bv"):
        assert (got[k] == 7.0).all(), k
    assert (got["grad_src"] == 0).all()
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST", "force")
    N, S, _, _, L, Lq, P = d["dims"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # head_dim 30 is no power of two: the constructor says so
        mod = MSDeformAttn(M * D, L, M, P).to(dev)
    calls = _lib.census(True)
    try:
        out, _, _ = mod(torch.randn(N, Lq, M * D, device=dev), torch.rand(N, Lq, L, 2, device=dev), d["src"].to(dev).requires_grad_(True),
                        d["shapes"].to(dev), d["lsi"].to(dev), None)
        out.sum().backward()
    finally:
        _lib.census(False)
    assert calls.get("ocpg_msda_fwd_f32", 0) == 1 and calls.get("ocpg_msda_bwd_f32", 0) == 1, calls
    assert not any(k.startswith("ocpg_msda_sf_") for k in calls), calls


SF_SYMS = ("ocpg_msda_sf_fwd_f32", "ocpg_msda_sf_bwd_f32", "ocpg_msda_sf_bwd_params_f32")


@pytest.mark.parametrize("mode,fwd", [("force", True), ("force", False), ("0", False)])
def test_module_and_transformer_reference_vectors(golden, dev, mode, fwd, monkeypatch):
    """the reference's module / transformer vectors at head_dim 32 with the cross-attention calls forced through the new kernels (the
    fixtures are far below the size at which the default rule takes them), and with the switch off"""
    from ocpg_amd import _lib
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST", mode)
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST_FWD", fwd)      # (off: the backward forms s / beta with the forward kernel, so all three show)
    for check, name, tol in ((mc.check_msda_module, "msda_module_d32", dict(rtol=2e-4, atol=2e-5)),
                             (mc.check_transformer, "transformer_d32", dict(rtol=5e-4, atol=5e-5))):
        calls = _lib.census(True)
        try:
            check(golden(name), dev, **tol)
        finally:
            _lib.census(False)
        for sym in SF_SYMS:
            assert (calls.get(sym, 0) >= 1) == (mode == "force"), (name, sym, calls)


def test_default_rule_leaves_fixture_sizes_alone(golden, dev, monkeypatch):
    from ocpg_amd import _lib
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST", "1")
    calls = _lib.census(True)
    try:
        mc.check_msda_module(golden("msda_module_d32"), dev, rtol=2e-4, atol=2e-5)
    finally:
        _lib.census(False)
    assert not any(k.startswith("ocpg_msda_sf_") for k in calls), calls


@pytest.mark.parametrize("fwd", [True, False])
def test_capture_and_replay(dev, fwd, monkeypatch):
    """the module's forward + backward at the first case's shape as a HIP graph on a side stream, replayed with refreshed src / query:
    equal to eager to 0 wherever the summation order is fixed, to the fp32-order floor in grad_src (float atomics)"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import MSDeformAttn
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST", "force")
    monkeypatch.setattr(_mda(), "SAMPLE_FIRST_FWD", fwd)
    d = _inputs(**CASE1, seed=5)
    N, S, M, D, L, Lq, P = d["dims"]
    C = M * D
    torch.manual_seed(0)
    mod = MSDeformAttn(C, L, M, P).to(dev)
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.02)
        mod.attention_weights.weight.normal_(0, 0.1)
        mod.value_proj.bias.normal_(0, 0.5)
    sh, lsi, pad = d["shapes"].to(dev), d["lsi"].to(dev), d["pad"].to(dev)
    sh._ocpg_host = d["shapes"]
    ref_pts = torch.rand(N, Lq, L, 2, device=dev)
    go = d["go"].to(dev)
    src = d["src"].to(dev).requires_grad_(True)
    query = torch.randn(N, Lq, C, device=dev).requires_grad_(True)

    def step():
        out, loc, attn = mod(query, ref_pts, src, sh, lsi, pad)
        return (out,) + torch.autograd.grad((out * go).sum(), [loc, attn, mod.value_proj.weight, mod.value_proj.bias, src])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        static = step()
    n = ctypes.c_int(-1)         # memset nodes (if torch captured any) become kernel nodes, as in the benchmark's graph step
    _lib.check(_lib.lib().ocpg_graph_replace_memsets(g.raw_cuda_graph(), ctypes.byref(n)), "ocpg_graph_replace_memsets")
    g.instantiate()
    gen = torch.Generator().manual_seed(99)
    for rep in range(2):
        with torch.no_grad():
            src.copy_(torch.randn(N, S, C, generator=gen))
            query.copy_(torch.randn(N, Lq, C, generator=gen))
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        for k, a, b in zip(("out", "grad_loc", "grad_attn", "grad_wv", "grad_bv"), got, want):
            assert torch.equal(a, b), (rep, k, (a - b).abs().max().item())
        e = _dist(got[5], want[5].double())
        print(f"replay {rep}: grad_src graph vs eager {e:.3e}")
        assert e <= FLOOR, (rep, e)
