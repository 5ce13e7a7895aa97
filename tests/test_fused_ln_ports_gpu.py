"""The extra ports of the dropout + add + LayerNorm kernels (csrc/fused_ln.hip: ocpg_dropout_add_ln_fwd_ex / _bwd_ex) and the model
plumbing that uses them (OCPG_FUSED_LN_PORTS).

Kernel level, through ctypes: the _ex symbols against the un-suffixed ones (bit for bit) and against torch's fp32 add / cast of the
stored `y`; the bias-gradient partials against the fp64 column sum of the stored gx with the worst-case bound of an fp32 sum of R
terms, gamma_R = R u / (1 - R u), u = 2^-24 (any summation order; the test itself sums the slots in fp64).

Module level: one encoder and one decoder layer, switch on against switch off from the same generator states.  Gradients whose backward
does not pass MSDeformAttn's atomic scatter are compared bit for bit (the same kernels run on the same bits), the two bias gradients the
norm kernels now form against the fp64 column sum with the gamma_R bound, and the rest within twice the distance of two switch-off runs."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SHAPES = [(1, 4), (5, 64), (7, 260), (50, 256), (9, 512), (6, 1024), (5, 2048), (4101, 256)]
SEED, OFFSET, EPS = 1234567, 7, 1e-5


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Case:
    def __init__(self, dev, r, c, xdtype, p):
        g = torch.Generator(device="cpu").manual_seed(r * 4099 + c)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
        self.dev, self.r, self.c, self.p = dev, r, c, p
        self.x = rnd(r, c).to(xdtype)
        self.res = rnd(r, c)
        self.gamma = (rnd(c) * 0.2 + 1.0).contiguous()
        self.beta = (rnd(c) * 0.2).contiguous()
        self.addend = rnd(r, c)
        self.g = [rnd(r, c) for _ in range(3)]

    def st(self):
        return torch.cuda.current_stream().cuda_stream

    def fwd(self, ex, addend=None, want_add=False, lp=None):
        from ocpg_amd._lib import lib
        r, c, dev = self.r, self.c, self.dev
        y, mean, rstd = _nan((r, c), torch.float32, dev), _nan((r,), torch.float32, dev), _nan((r,), torch.float32, dev)
        y_add = _nan((r, c), torch.float32, dev) if want_add else None
        y_lp = _nan((r, c), lp, dev) if lp is not None else None
        head = (self.x.data_ptr(), self.res.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), r, c, EPS, self.p, SEED, OFFSET, None,
                DT[self.x.dtype], y.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        if ex:
            rc = lib().ocpg_dropout_add_ln_fwd_ex(*head, _ptr(addend), _ptr(y_add), _ptr(y_lp), 0 if lp is None else DT[lp], self.st())
        else:
            rc = lib().ocpg_dropout_add_ln_fwd(*head, self.st())
        return rc, y, mean, rstd, y_add, y_lp

    def bwd(self, ex, gs, mean, rstd, want_sum=False, dtypes=None):
        """gs: 1..3 gradient tensors (None entries allowed after the first)"""
        from ocpg_amd._lib import lib
        r, c, dev = self.r, self.c, self.dev
        slots = lib().ocpg_dropout_add_ln_bwd_slots(r)
        gx, gres = _nan((r, c), self.x.dtype, dev), _nan((r, c), torch.float32, dev)
        part = _nan((slots, 2, c), torch.float32, dev)
        gxsum = _nan((slots, c), torch.float32, dev) if want_sum else None
        tail = (self.x.data_ptr(), self.res.data_ptr(), self.gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), r, c, self.p, SEED, OFFSET, None,
                DT[self.x.dtype], gx.data_ptr(), gres.data_ptr(), part.data_ptr())
        if ex:
            gs = list(gs) + [None] * (3 - len(gs))
            ga = []
            for i, g in enumerate(gs):
                ga += [_ptr(g), (0 if g is None else DT[g.dtype]) if dtypes is None else dtypes[i]]
            rc = lib().ocpg_dropout_add_ln_bwd_ex(*ga, *tail, _ptr(gxsum), self.st())
        else:
            rc = lib().ocpg_dropout_add_ln_bwd(gs[0].data_ptr(), *tail, self.st())
        return rc, gx, gres, part, gxsum


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("r,c", SHAPES)
def test_ports_kernels(dev, r, c, xdtype, p):
    k = _Case(dev, r, c, xdtype, p)
    # 1. no extras: the un-suffixed kernel, bit for bit
    rc0, y0, mean0, rstd0, _, _ = k.fwd(False)
    rc1, y1, mean1, rstd1, _, _ = k.fwd(True)
    assert rc0 == 0 and rc1 == 0
    assert not torch.isnan(y0).any()
    assert _same_bits(y0, y1) and _same_bits(mean0, mean1) and _same_bits(rstd0, rstd1)
    # 2. y + addend as torch's fp32 add, y in 16 bits as torch's cast; every element written
    for lp in (torch.bfloat16, torch.float16):
        rc, y, mean, rstd, y_add, y_lp = k.fwd(True, k.addend, True, lp)
        assert rc == 0
        assert _same_bits(y, y0) and _same_bits(mean, mean0) and _same_bits(rstd, rstd0)
        assert not torch.isnan(y_add).any() and not torch.isnan(y_lp.float()).any()
        assert _same_bits(y_add, y0 + k.addend)
        assert _same_bits(y_lp, y0.to(lp))
    rc, y, _, _, y_add, y_lp = k.fwd(True, k.addend, True, None)       # each port on its own
    assert rc == 0 and _same_bits(y, y0) and _same_bits(y_add, y0 + k.addend)
    rc, y, _, _, _, y_lp = k.fwd(True, None, False, torch.bfloat16)
    assert rc == 0 and _same_bits(y, y0) and _same_bits(y_lp, y0.to(torch.bfloat16))
    # 3. fp32 g0 only: the un-suffixed kernel, bit for bit
    rc0, gx0, gres0, part0, _ = k.bwd(False, [k.g[0]], mean0, rstd0)
    rc1, gx1, gres1, part1, _ = k.bwd(True, [k.g[0]], mean0, rstd0)
    assert rc0 == 0 and rc1 == 0
    assert not torch.isnan(gx0.float()).any() and not torch.isnan(gres0).any() and not torch.isnan(part0).any()
    assert _same_bits(gx0, gx1) and _same_bits(gres0, gres1) and _same_bits(part0, part1)
    # 4. two and three addends, every dtype in every position: the un-suffixed kernel on gy = (g0 + g1) + g2
    dts = (torch.float32, torch.bfloat16, torch.float16)
    for n in (2, 3):
        for combo in itertools.product(dts, repeat=n):
            gs = [g.to(d) for g, d in zip(k.g, combo)]
            gy = gs[0].float() + gs[1].float()
            if n == 3:
                gy = gy + gs[2].float()
            rc0, gxr, gresr, partr, _ = k.bwd(False, [gy], mean0, rstd0)
            rc1, gxe, grese, parte, _ = k.bwd(True, gs, mean0, rstd0)
            assert rc0 == 0 and rc1 == 0
            assert _same_bits(gxr, gxe) and _same_bits(gresr, grese) and _same_bits(partr, parte), (n, combo)
    # 5. the bias-gradient partials: column sums of gx as stored
    gs = [k.g[0], k.g[1].to(torch.bfloat16)]
    rc, gx, gres, part, gxsum = k.bwd(True, gs, mean0, rstd0, want_sum=True)
    rc0, gxr, gresr, partr, _ = k.bwd(False, [gs[0] + gs[1].float()], mean0, rstd0)
    assert rc == 0 and rc0 == 0
    assert _same_bits(gx, gxr) and _same_bits(gres, gresr) and _same_bits(part, partr)
    assert not torch.isnan(gxsum).any()
    u = r * 2.0 ** -24
    gamma_r = u / (1.0 - u)
    diff = (gxsum.double().sum(0) - gx.double().sum(0)).abs()
    bound = gamma_r * gx.double().abs().sum(0)
    print("gxsum max |diff| %.3e, max bound %.3e" % (diff.max().item(), bound.max().item()))
    assert (diff <= bound).all()


def test_ports_argument_errors(dev):
    k = _Case(dev, 5, 64, torch.float32, 0.1)
    rc, y, mean, rstd, _, _ = k.fwd(True)
    assert rc == 0
    assert k.fwd(True, k.addend, False, None)[0] <= -1000            # addend without y_add
    from ocpg_amd._lib import lib
    y_add = torch.empty(5, 64, device=dev)
    head = (k.x.data_ptr(), k.res.data_ptr(), k.gamma.data_ptr(), k.beta.data_ptr(), 5, 64, EPS, 0.1, SEED, OFFSET, None, 0, y.data_ptr(),
            mean.data_ptr(), rstd.data_ptr())
    assert lib().ocpg_dropout_add_ln_fwd_ex(*head, None, y_add.data_ptr(), None, 0, k.st()) <= -1000      # y_add without addend
    y_lp = torch.empty(5, 64, device=dev, dtype=torch.bfloat16)
    assert lib().ocpg_dropout_add_ln_fwd_ex(*head, None, None, y_lp.data_ptr(), 0, k.st()) <= -1000       # 16-bit port, fp32 code
    assert lib().ocpg_dropout_add_ln_fwd_ex(*head, None, None, y_lp.data_ptr(), 3, k.st()) <= -1000
    assert k.bwd(True, [k.g[0]], mean, rstd, dtypes=[3, 0, 0])[0] <= -1000                               # bad dtype codes
    assert k.bwd(True, [k.g[0], k.g[1]], mean, rstd, dtypes=[0, -1, 0])[0] <= -1000
    assert k.bwd(True, [None, k.g[1]], mean, rstd)[0] <= -1000                                            # NULL g0
    torch.cuda.synchronize()


# ---- module level ---------------------------------------------------------------------------------------------------------------------
LEVELS = [(20, 28), (10, 14), (5, 7), (3, 4)]
# LQ: decoder queries.  40 keeps the layer on its few-row kernels (80 rows) and its self-attention on the HIP attention kernels, and
# gives MSDeformAttn's backward about 10 000 atomic adds onto 3 000 (token, head) rows: enough collisions that the run-to-run distance
# below is a sum over many elements (with 10 queries two switch-off runs differed in one element, and the "twice the spread" check
# compared counts of one, two or three flipped roundings: it failed one run in three on bit-identical inputs)
D_MODEL, D_FFN, HEADS, N, LQ = 64, 128, 2, 2, 40
ENC_PLAIN = ("norm2.", "linear2.", "linear1.", "norm1.", "self_attn.output_proj.")      # backward does not pass MSDeformAttn's scatter
DEC_PLAIN = ("norm3.", "linear2.", "linear1.", "norm1.", "cross_attn.output_proj.")


def _geometry(dev):
    host = torch.tensor(LEVELS, dtype=torch.long)
    starts = torch.cat((host.new_zeros(1), host.prod(1).cumsum(0)[:-1]))
    shapes, ls = host.to(dev), starts.to(dev)
    shapes._ocpg_host, ls._ocpg_host = host, starts
    return shapes, ls


def _setup(kind, dev):
    from ocpg_amd.models import deformable_transformer as dt
    torch.manual_seed(3)
    s = sum(h * w for h, w in LEVELS)
    cls = dt.DeformableTransformerEncoderLayer if kind == "enc" else dt.DeformableTransformerDecoderLayer
    layer = cls(D_MODEL, D_FFN, 0.1, "relu", len(LEVELS), HEADS, 4).to(dev).train()
    with torch.no_grad():                       # the zero-initialised query projections would leave their inputs without a gradient
        for n_, p_ in layer.named_parameters():
            if "sampling_offsets.weight" in n_ or "attention_weights" in n_:
                p_.normal_(0, 0.05)
    shapes, ls = _geometry(dev)
    ins = {"src": torch.randn(N, s, D_MODEL, device=dev, requires_grad=True)}
    if kind == "enc":
        ins["pos"] = torch.randn(N, s, D_MODEL, device=dev, requires_grad=True)
        ref = torch.rand(N, s, len(LEVELS), 2, device=dev)
        ins["go"] = torch.randn(N, s, D_MODEL, device=dev)
    else:
        ins["tgt"] = torch.randn(N, LQ, D_MODEL, device=dev, requires_grad=True)
        ins["query_embed"] = torch.randn(LQ, D_MODEL, device=dev, requires_grad=True)
        ref = torch.rand(N, LQ, len(LEVELS), 2, device=dev)
        ins["go"] = torch.randn(N, LQ, D_MODEL, device=dev)
    return layer, ins, ref, shapes, ls


def _run(kind, layer, ins, ref, shapes, ls, amp, ports, states, monkeypatch, on_colsum=None):
    from ocpg_amd import _lib
    from ocpg_amd.models import amp_cache
    from ocpg_amd.models.ops.functions import fused_ln_func
    torch.set_rng_state(states[0]), torch.cuda.set_rng_state(states[1]), fused_ln_func.set_rng_state(states[2])
    for m in layer.modules():
        if hasattr(m, "_sel_state"):
            m._sel_state.zero_()
    monkeypatch.setattr(fused_ln_func, "PORTS", ports)
    real_colsum = amp_cache.colsum
    if on_colsum is not None:
        def colsum(gy2, like):
            on_colsum(gy2)
            return real_colsum(gy2, like)
        monkeypatch.setattr(amp_cache, "colsum", colsum)
    leaves = [t for t in ins.values() if t.requires_grad] + list(layer.parameters())
    for t in leaves:
        t.grad = None
    calls = _lib.census(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        if kind == "enc":
            out = layer(ins["src"], ins["pos"], ref, shapes, ls)
        else:
            out = layer(ins["tgt"], ins["query_embed"][None].expand(N, -1, -1), ref, ins["src"], shapes, ls)[0]
    fwd_calls = dict(calls)
    (out.float() * ins["go"]).sum().backward()
    _lib.census(False)
    monkeypatch.setattr(amp_cache, "colsum", real_colsum)
    bwd_calls = {s_: n_ - fwd_calls.get(s_, 0) for s_, n_ in calls.items()}
    grads = {n_: p_.grad.detach().clone() for n_, p_ in layer.named_parameters()}
    grads.update({"input." + n_: t.grad.detach().clone() for n_, t in ins.items() if t.requires_grad})
    return out.detach().clone(), grads, dict(calls), bwd_calls


@pytest.mark.parametrize("amp", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_layer_switch_on_equals_off(dev, kind, amp, monkeypatch):
    from ocpg_amd.models import amp_cache
    from ocpg_amd.models.ops.functions import fused_ln_func
    monkeypatch.setattr(amp_cache, "TOKEN_LINEAR_MIN_ROWS", 1024)
    layer, ins, ref, shapes, ls = _setup(kind, dev)
    rows = N * sum(h * w for h, w in LEVELS)
    assert rows == 1494
    args = (kind, layer, ins, ref, shapes, ls, amp)
    states = (torch.get_rng_state(), torch.cuda.get_rng_state(), fused_ln_func.get_rng_state())
    _run(*args, False, states, monkeypatch)                 # first use of every GEMM shape (plans are chosen there)
    records = []                                            # (fp64 column sum, fp64 column sum of magnitudes) of every bias-gradient input
    out_a, g_a, calls_a, bwd_a = _run(*args, False, states, monkeypatch, lambda gy2: records.append((gy2.double().sum(0), gy2.double().abs().sum(0))))
    out_b, g_b, calls_b, bwd_b = _run(*args, False, states, monkeypatch)
    out_on, g_on, calls_on, bwd_on = _run(*args, True, states, monkeypatch)

    assert _same_bits(out_a, out_b) and _same_bits(out_a, out_on)
    # census: the _ex symbols with the switch on (also counted under the old names), none with it off
    for sym in ("ocpg_dropout_add_ln_fwd_ex", "ocpg_dropout_add_ln_bwd_ex"):
        assert calls_on.get(sym, 0) >= 1 and calls_a.get(sym, 0) == 0, (sym, calls_on, calls_a)
    assert calls_on["ocpg_dropout_add_ln_fwd"] == calls_a["ocpg_dropout_add_ln_fwd"] == (2 if kind == "enc" else 3)
    assert calls_on["ocpg_dropout_add_ln_fwd_ex"] == calls_on["ocpg_dropout_add_ln_fwd"]
    if kind == "enc":
        # output_proj's and linear2's bias gradients come out of the norm kernels' backward: two column-sum calls less (value_proj and
        # the query projection keep theirs)
        assert len(records) >= 2
        n_off = len(records)
        seen = []
        _run(*args, True, states, monkeypatch, lambda gy2: seen.append(gy2.shape))
        assert len(seen) == n_off - 2, (seen, n_off)
        assert bwd_on.get("ocpg_colsum_partials", 0) <= bwd_a.get("ocpg_colsum_partials", 0)

    plain = ENC_PLAIN if kind == "enc" else DEC_PLAIN
    u = rows * 2.0 ** -24
    gamma_r = u / (1.0 - u)
    rest_spread, rest_dist = 0.0, 0.0
    for name in sorted(g_a):
        a, b, on = g_a[name], g_b[name], g_on[name]
        if name.startswith(plain):
            fused_bias = kind == "enc" and name in ("linear2.bias", "self_attn.output_proj.bias")
            if not fused_bias:
                # same kernels on the same bits in the same order: nothing is re-associated
                assert _same_bits(a, on), name
                continue
            # a re-ordered fp32 sum of `rows` terms (then, under autocast, one rounding to bf16): against the fp64 column sum of the
            # very gradient matrix the switch-off run summed (the record nearest to its result)
            ref_sum, ref_abs = min(records, key=lambda r_: (r_[0].float() - a).abs().max().item() if r_[0].shape == a.shape else float("inf"))
            lp_round = 2.0 ** -8 if (amp and name == "linear2.bias") else 0.0
            for g in (a, on):
                bound = gamma_r * ref_abs + lp_round * (ref_sum.abs() + gamma_r * ref_abs)
                assert ((g.double() - ref_sum).abs() <= bound).all(), name
            continue
        # The rest: behind MSDeformAttn's atomic scatter.  What separates two runs there is the rounding of atomic adds that landed in
        # another order: a property of the run, which at these sizes shows in a handful of elements (seen on the GPU, decoder layer,
        # cross_attn.value_proj.bias: two switch-off runs 1 element x 1 ulp apart, on-vs-off 2-3 elements x 1-2 ulp, from bit-identical
        # inputs of that backward -- the switch moves allocations and launch times, two identical runs share them).  One tensor's pair
        # of runs is too small a sample of it, so the distances (2-norm relative to the tensor's, as in the project's output
        # comparisons) are pooled over the group: the largest on-vs-off distance against twice the largest off-vs-off one.
        scale = a.double().norm().item()
        spread = (a.double() - b.double()).norm().item() / scale
        dist = (on.double() - a.double()).norm().item() / scale
        print("%-44s off-vs-off %.3e  on-vs-off %.3e  (largest element: %.3e, %.3e)" % (name, spread, dist, (a - b).abs().max().item(),
                                                                                         (on - a).abs().max().item()))
        rest_spread, rest_dist = max(rest_spread, spread), max(rest_dist, dist)
    print("behind the atomic scatter: largest off-vs-off %.3e, largest on-vs-off %.3e" % (rest_spread, rest_dist))
    assert rest_dist <= 2.0 * rest_spread
