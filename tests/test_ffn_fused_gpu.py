"""The encoder FFN's bias + ReLU + dropout passes as GEMM epilogues (csrc/gemm_dgrad_bn.hip: ocpg_gemm_bias_relu_dropout_fwd,
ocpg_gemm_dgrad_mask; fused_ln_func.FFN_FUSED_FWD / FFN_FUSED_BWD): both kernels against fp64 on the bf16-rounded operands with
elementwise bounds, the autograd chain with the switch on and off, the guard against a second consumer of the hidden map, and a captured
step under GraphRng.

Bounds.  An output is one fp32 chain over k, one or two fp32 operations and ONE rounding to bf16:
    |got - ref| <= 2^-8 |ref| + 2^-20 sum_k |x_mk w_nk|
(2^-8: one bf16 rounding moves a value by at most half a spacing, 2^-8 of its magnitude; 2^-20 of the sum of magnitudes: a loose cover of an fp32 accumulation of <= 256 terms,
whose first-order worst case is K 2^-24 = 2^-16 and whose typical size is sqrt(K) 2^-24 = 2^-20).  A partial column sum adds fp32 values of
g[m, n] that each carry that accumulation error, so its bound is 2^-20 of the sum of magnitudes of every product that enters the column:
sum over the unmasked rows m and over k of |a_mk w_kn| scale."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(m, n, k) for m in (1, 127, 129, 300) for n, k in ((128, 128), (256, 256))] + [(129, 2048, 256)]
PS = (0.0, 0.1, 0.5)
RNG = (20240607, 11)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _probe_keep(rows, cols, p, rng, dev):
    """The keep pattern (1/(1-p) or 0) brd_fwd draws for (seed, offset) on a [rows, cols] map: the existing kernel on an all-ones
    pre-activation (fp32, K = 1: the pair's route)."""
    from ocpg_amd.models.ops.functions import fused_ln_func as f
    if p == 0:
        return torch.ones(rows, cols, device=dev)
    return f.LinearBiasReluDropout.apply(torch.ones(rows, 1, device=dev), torch.ones(cols, 1, device=dev), torch.zeros(cols, device=dev), p, rng, 1)


_OPERANDS = {}


def _operands(m, n, k, dev):
    """Shared, never modified: x [m,k], w1 [n,k] (linear1's layout), bias [n], a [m,k] (a gradient), w2 [k,n] (linear2's layout), and the
    fp64 products with their sums of magnitudes."""
    key = (m, n, k)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * m + n + k)
        bf = torch.bfloat16
        x = torch.randn(m, k, generator=g).to(dev, bf)
        w1 = (0.2 * torch.randn(n, k, generator=g)).to(dev, bf)
        b = torch.randn(n, generator=g).to(dev, bf)
        a = torch.randn(m, k, generator=g).to(dev, bf)
        w2 = (0.2 * torch.randn(k, n, generator=g)).to(dev, bf)
        hmap = torch.relu(torch.randn(m, n, generator=g)).to(dev, bf)
        _OPERANDS[key] = dict(x=x, w1=w1, b=b, a=a, w2=w2, hmap=hmap,
                              pre=x.double() @ w1.double().t() + b.double(), pre_abs=x.double().abs() @ w1.double().abs().t(),
                              v=a.double() @ w2.double(), v_abs=a.double().abs() @ w2.double().abs())
    return _OPERANDS[key]


def _fwd(o, p, rng, h, tile, round_gemm=0):
    from ocpg_amd._lib import lib, stream_ptr
    m, k = o["x"].shape
    n = o["w1"].shape[0]
    return lib().ocpg_gemm_bias_relu_dropout_fwd(o["x"].data_ptr(), o["w1"].data_ptr(), o["b"].data_ptr(), p, rng[0], rng[1], None, h.data_ptr(),
                                                 m, n, k, 1, tile, round_gemm, stream_ptr())


def _bwd(o, mask, scale, out, part, tile):
    from ocpg_amd._lib import lib, stream_ptr
    m, k = o["a"].shape
    n = o["w2"].shape[1]
    return lib().ocpg_gemm_dgrad_mask(o["a"].data_ptr(), o["w2"].data_ptr(), mask.data_ptr(), scale, out.data_ptr(), part.data_ptr(), m, n, k, 1,
                                      tile, stream_ptr())


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_forward_kernel_against_fp64(dev, m, n, k, p):
    o = _operands(m, n, k, dev)
    keep = _probe_keep(m, n, p, RNG, dev).double()
    assert torch.all((keep == 0) | ((keep - 1 / (1 - p)).abs() < 1e-6))
    ref = torch.relu(o["pre"]) * keep
    acc = 2.0 ** -20 * o["pre_abs"]
    unsure = o["pre"].abs() <= acc                  # may fall on either side of the ReLU
    assert unsure.double().mean().item() <= 1e-3
    for tile in (0, 1, 2):
        h = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device=dev)
        assert _fwd(o, p, RNG, h, tile) == 0
        torch.cuda.synchronize()
        got = h.double()
        assert not torch.isnan(got).any(), tile
        assert torch.all(got[keep == 0] == 0), tile                      # the zero pattern of the dropped elements, exactly
        err, bound = (got - ref).abs(), 2.0 ** -8 * ref.abs() + acc
        print("fwd tile %d: largest error / bound %.3f, left out %d" % (tile, (err / bound.clamp_min(1e-300))[~unsure & (bound > 0)].max().item()
                                                                        if (~unsure & (bound > 0)).any() else 0.0, int(unsure.sum())))
        assert torch.all((err <= bound) | unsure), (tile, (err - bound)[~unsure].max().item())


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_backward_kernel_against_fp64(dev, m, n, k, p):
    o = _operands(m, n, k, dev)
    keep = _probe_keep(m, n, p, RNG, dev)
    hmap = (o["hmap"].float() * keep).to(torch.bfloat16)                 # a saved hidden map: zero where ReLU or dropout zeroed it
    scale = 1.0 / (1.0 - p)
    on = (hmap > 0).double()
    ref = o["v"] * scale * on
    acc = 2.0 ** -20 * o["v_abs"]
    results = []
    for tile, tm in ((0, 128), (1, 64), (2, 64)):
        mt = (m + tm - 1) // tm
        outs = []
        for _ in range(2):
            out = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device=dev)
            part = torch.full((mt, n), float("nan"), dtype=torch.float32, device=dev)
            assert _bwd(o, hmap, scale, out, part, tile) == 0
            torch.cuda.synchronize()
            outs.append((out, part))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), tile       # two calls: the same bits
        out, part = outs[0]
        assert not torch.isnan(out.float()).any() and not torch.isnan(part).any(), tile
        err, bound = (out.double() - ref).abs(), 2.0 ** -8 * ref.abs() + acc * on
        assert torch.all(err <= bound), (tile, (err - bound).max().item())
        cs_err = (part.double().sum(0) - ref.sum(0)).abs()
        cs_bound = 2.0 ** -20 * (o["v_abs"] * scale * on).sum(0)
        print("bwd tile %d: largest out error / bound %.3f, colsum %.3f" % (tile, (err / bound.clamp_min(1e-300))[bound > 0].max().item()
                                                                            if (bound > 0).any() else 0.0,
                                                                            (cs_err / cs_bound.clamp_min(1e-300))[cs_bound > 0].max().item()
                                                                            if (cs_bound > 0).any() else 0.0))
        assert torch.all(cs_err <= cs_bound), (tile, (cs_err - cs_bound).max().item())
        results.append(out)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])                 # every tile: the same bits


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_forward_kernel_rounding_like_the_pair(dev, m, n, k, p):
    """round_gemm = 1 (what the step runs): h = bf16(max(bf16(v) + bias, 0) keep), the pair's arithmetic.
    Against fp64: a second rounding, of v = x w^T, enters before the bias: |got - ref| <= 2^-8 |ref| + (2^-8 |v| + 2^-20 sum_k |x w|) keep,
    and a pre-activation within 2^-8 |v| + 2^-20 sum_k |x w| of zero may fall on either side of the ReLU (left out; with v ~ N(0, 3.2^2) + bias
    that is about 2^-8 * 2.5 * 2 * 0.12 = 0.25 % of the elements: at most 2 %).
    Against the pair itself (hipBLASLt GEMM + brd_fwd, same (seed, offset)): the same bits wherever both GEMMs' fp32 sums round to the
    same bf16 value.  Two fp32 sums of the same products differ by at most 2 * 2^-20 sum|x w| (the accumulation term above, once each), the
    spacing of bf16 at v is >= 2^-8 |v|, so the chance that a rounding boundary lies between them is about 2^-12 sum|x w| / |v|: 1e-3 for
    sum|x w| / |v| ~ 4 at K = 256 as a worst case, 1e-4 typically: at most 0.2 % of the elements (2 on the smallest maps) may differ, each by at most one spacing of
    bf16(v) through the ReLU and the keep factor plus one rounding of h: 2^-7 |bf16(v)| keep + 2^-7 |h|."""
    from ocpg_amd._lib import lib, stream_ptr
    o = _operands(m, n, k, dev)
    keep = _probe_keep(m, n, p, RNG, dev).double()
    v = o["pre"] - o["b"].double()
    ref = torch.relu(o["pre"]) * keep
    slack = 2.0 ** -8 * v.abs() + 2.0 ** -20 * o["pre_abs"]
    unsure = o["pre"].abs() <= slack
    assert unsure.double().mean().item() <= 2e-2
    pair = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    L = lib()
    assert L.ocpg_gemm(o["x"].data_ptr(), o["w1"].data_ptr(), pair.data_ptr(), None, 1, 1, 0, 1, m, n, k, k, k, n, 1, 0, 0, 0, 1.0, 0.0, stream_ptr()) == 0
    a_pair = pair.double()
    assert L.ocpg_bias_relu_dropout_fwd(pair.data_ptr(), o["b"].data_ptr(), m, n, p, RNG[0], RNG[1], None, 1, pair.data_ptr(), stream_ptr()) == 0
    for tile in (0, 1, 2):
        h = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device=dev)
        assert _fwd(o, p, RNG, h, tile, 1) == 0
        torch.cuda.synchronize()
        got = h.double()
        assert not torch.isnan(got).any(), tile
        assert torch.all(got[keep == 0] == 0), tile
        err, bound = (got - ref).abs(), 2.0 ** -8 * ref.abs() + slack * keep
        assert torch.all((err <= bound) | unsure), (tile, (err - bound)[~unsure].max().item())
        differ = got != pair.double()
        print("fwd (rounding) tile %d: %d of %d elements differ from the pair's" % (tile, int(differ.sum()), differ.numel()))
        assert int(differ.sum()) <= max(2, 2e-3 * differ.numel()), (tile, int(differ.sum()))     # (a map of 128 elements: 2 of them)
        d_bound = 2.0 ** -7 * a_pair.abs() * keep + 2.0 ** -7 * pair.double().abs()
        assert torch.all((got - pair.double()).abs() <= d_bound), tile


def test_declines_like_dgrad_bn(dev):
    o = _operands(127, 128, 128, dev)
    from ocpg_amd._lib import lib, stream_ptr
    L = lib()
    h = torch.empty(127, 128, dtype=torch.bfloat16, device=dev)
    part = torch.empty(2, 128, device=dev)
    x, w1, b, a, w2 = (o[n_].data_ptr() for n_ in ("x", "w1", "b", "a", "w2"))
    st = stream_ptr()
    assert L.ocpg_gemm_bias_relu_dropout_fwd(x, w1, b, 0.0, 1, 1, None, h.data_ptr(), 127, 128, 64, 1, 0, 0, st) == -2000       # K % 128
    assert L.ocpg_gemm_bias_relu_dropout_fwd(x, w1, b, 0.0, 1, 1, None, h.data_ptr(), 127, 64, 128, 1, 0, 0, st) == -2000       # N % tile width
    assert L.ocpg_gemm_bias_relu_dropout_fwd(x + 2, w1, b, 0.0, 1, 1, None, h.data_ptr(), 126, 128, 128, 1, 0, 0, st) == -2001
    assert L.ocpg_gemm_bias_relu_dropout_fwd(x, w1, b, 0.0, 1, 1, None, h.data_ptr(), 127, 128, 128, 2, 0, 0, st) == -2002       # fp16: the pair
    assert L.ocpg_gemm_dgrad_mask(a, w2, h.data_ptr(), 1.0, h.data_ptr(), part.data_ptr(), 127, 128, 64, 1, 0, st) == -2000
    assert L.ocpg_gemm_dgrad_mask(a, w2, h.data_ptr(), 1.0, h.data_ptr(), part.data_ptr() + 4, 127, 128, 128, 1, 0, st) == -2001
    assert L.ocpg_gemm_dgrad_mask(a, w2, h.data_ptr(), 1.0, h.data_ptr(), part.data_ptr(), 127, 128, 128, 0, 0, st) == -2002


# ---- autograd chain: LinearBiasReluDropout -> linear_dropout_add_layer_norm ----------------------------------------------------------
ROWS, C, P = 8200, 256, 0.1           # ragged against the 128-row tile; at amp_cache.TOKEN_LINEAR_MIN_ROWS (8192) and above


def _chain_inputs(dev):
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    t = dict(x=torch.randn(ROWS, C, generator=g).to(dev, bf), w1=(0.2 * torch.randn(C, C, generator=g)).to(dev, bf),
             b1=torch.randn(C, generator=g).to(dev, bf), w2=(0.2 * torch.randn(C, C, generator=g)).to(dev, bf),
             b2=torch.randn(C, generator=g).to(dev, bf), res=torch.randn(ROWS, C, generator=g).to(dev), go=torch.randn(ROWS, C, generator=g).to(dev))
    norm = torch.nn.LayerNorm(C).to(dev)
    return t, norm


def _chain(t, norm, fused, monkeypatch, p=P, rng=RNG, extra_consumer=False, exact=True):
    """-> (h, gx, gw, gb) of the first Linear, and the call census"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import fused_ln_func as f
    monkeypatch.setattr(f, "FFN_FUSED_FWD", fused)
    monkeypatch.setattr(f, "FFN_FUSED_BWD", fused)
    monkeypatch.setattr(f, "FFN_FWD_EXACT", exact)
    x, w1, b1 = (t[n_].clone().requires_grad_(True) for n_ in ("x", "w1", "b1"))
    calls = _lib.census(True)
    try:
        h = f.LinearBiasReluDropout.apply(x, w1, b1, p, rng, 5)
        y = f.linear_dropout_add_layer_norm(h, t["w2"], t["b2"], t["res"], norm, 0.0, rng=rng)[0]
        loss = (y * t["go"]).sum()
        if extra_consumer:
            loss = loss + h.float().sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib.census(False)
    return [h.detach().double(), x.grad.double(), w1.grad.double(), b1.grad.double()], dict(calls)


def test_chain_switch_on_and_off_against_fp64(dev, monkeypatch):
    t, norm = _chain_inputs(dev)
    keep = _probe_keep(ROWS, C, P, RNG, dev).double()
    x, w1, b1 = (t[n_].double().requires_grad_(True) for n_ in ("x", "w1", "b1"))
    h = torch.relu(x @ w1.t() + b1) * keep
    y = torch.nn.functional.layer_norm(t["res"].double() + h @ t["w2"].double().t() + t["b2"].double(), (C,), norm.weight.double(), norm.bias.double(), norm.eps)
    (y * t["go"].double()).sum().backward()
    ref = [h.detach(), x.grad, w1.grad, b1.grad]
    on, calls_on = _chain(t, norm, True, monkeypatch)
    off, calls_off = _chain(t, norm, False, monkeypatch)
    for sym in ("ocpg_gemm_bias_relu_dropout_fwd", "ocpg_gemm_dgrad_mask"):
        assert calls_on.get(sym, 0) == 1 and calls_off.get(sym, 0) == 0, (sym, calls_on, calls_off)
    for sym in ("ocpg_bias_relu_dropout_fwd", "ocpg_bias_relu_dropout_bwd"):
        assert calls_off.get(sym, 0) == 1 and calls_on.get(sym, 0) == 0, (sym, calls_on, calls_off)
    for name, r, a, b in zip(("h", "gx", "gw", "gb"), ref, on, off):
        e_on, e_off = ((a - r).norm() / r.norm()).item(), ((b - r).norm() / r.norm()).item()
        print("%s: fused %.3e, pair %.3e (norm-relative to fp64)" % (name, e_on, e_off))
        assert e_on <= 1.25 * e_off, (name, e_on, e_off)         # the fused route drops roundings and adds none


def test_chain_default_form_keeps_the_pairs_hidden_map(dev, monkeypatch):
    """The step's default (the forward rounds the GEMM result as the pair does): h equals the pair's in all but 0.2 % of its elements (the
    bound of test_forward_kernel_rounding_like_the_pair), so no ReLU is decided differently beyond those, and the gradients of the fused
    route are no further from the pair's than the pair is from fp64 (2.3e-2 norm-relative at this shape, printed by the test above)."""
    t, norm = _chain_inputs(dev)
    on, calls_on = _chain(t, norm, True, monkeypatch, exact=False)
    off, _ = _chain(t, norm, False, monkeypatch)
    assert calls_on.get("ocpg_gemm_bias_relu_dropout_fwd", 0) == 1 and calls_on.get("ocpg_gemm_dgrad_mask", 0) == 1, calls_on
    differ = (on[0] != off[0]).double().mean().item()
    print("h: %.2e of the elements differ from the pair's" % differ)
    assert differ <= 2e-3
    for name, a, b in zip(("gx", "gw", "gb"), on[1:], off[1:]):
        d = ((a - b).norm() / b.norm()).item()
        print("%s: fused (default form) vs pair %.3e" % (name, d))
        assert d <= 2.3e-2, (name, d)


def test_second_consumer_of_hidden_map_raises(dev, monkeypatch):
    t, norm = _chain_inputs(dev)
    with pytest.raises(RuntimeError, match="OCPG_FFN_FUSED"):
        _chain(t, norm, True, monkeypatch, extra_consumer=True)
    _chain(t, norm, False, monkeypatch, extra_consumer=True)     # the pair serves such a graph


def test_chain_under_graph_replay(dev, monkeypatch):
    """A captured forward + backward with GraphRng: two replays draw different masks, the first equals the eager step on the same generator state."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import fused_ln_func as f
    monkeypatch.setattr(f, "FFN_FUSED_FWD", True)
    monkeypatch.setattr(f, "FFN_FUSED_BWD", True)
    t, norm = _chain_inputs(dev)
    x, w1, b1 = (t[n_].clone().requires_grad_(True) for n_ in ("x", "w1", "b1"))

    def step():
        h = f.LinearBiasReluDropout.apply(x, w1, b1, 0.25, None, 5)
        y = f.linear_dropout_add_layer_norm(h, t["w2"], t["b2"], t["res"], norm, 0.25)[0]
        gx, gw, gb = torch.autograd.grad((y * t["go"]).sum(), (x, w1, b1))
        return [v.detach().clone() for v in (h, y, gx, gw, gb)]

    saved = f.get_rng_state()
    try:
        f.set_rng_state({"dropout_calls": 500})
        calls = _lib.census(True)
        eager = [step() for _ in range(2)]
        _lib.census(False)
        assert calls.get("ocpg_gemm_bias_relu_dropout_fwd", 0) == 2 and calls.get("ocpg_gemm_dgrad_mask", 0) == 2, calls
        assert not torch.equal(eager[0][0], eager[1][0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                  # the library's GEMM workspace is per (device, stream): allocate it before the capture
        torch.cuda.synchronize()
        f.set_rng_state({"dropout_calls": 500})
        rng = f.GraphRng(dev)
        g = torch.cuda.CUDAGraph()
        with rng, torch.cuda.graph(g, stream=side):
            static = step()
            rng.advance()
        rng.finalize()
        assert rng.calls == 2
        replays = []
        for r in range(2):
            g.replay()
            rng.replayed()
            torch.cuda.synchronize()
            replays.append([v.clone() for v in static])
        for i, (got, want) in enumerate(zip(replays[0], eager[0])):
            assert torch.equal(got, want), (i, (got.float() - want.float()).abs().max().item())
        assert not torch.equal(replays[0][0], replays[1][0])
        assert torch.equal((replays[1][0] == 0), (eager[1][0] == 0))
    finally:
        f.set_rng_state(saved)
