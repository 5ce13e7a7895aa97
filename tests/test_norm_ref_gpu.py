"""csrc/layernorm.hip (ln_fwd / ln_bwd), csrc/fused_ln.hip (dal_fwd / dal_bwd) and csrc/groupnorm.hip (one-launch and pixel-tiled kernels)
against the fp64 reference of tests/norm_ref.py, every element of every output held to the bound derived there: |got - ref| <= bound, no
multiplier, no max|ref|, no other kernel as the yardstick (tests/test_norm_bounds_cpu.py shows what this harness sees and what the older
criterion does not).

(a) Through the C ABI (ctypes, output buffers pre-filled with NaN, return codes checked): y, mean, rstd, dx / gx / gres of every case and
    dtype, and dgamma / dbeta as the fp64 sum of the per-workgroup (ln, dal) or per-frame (gn) partials, under the chain bound of
    `geometry`.  The backward reads the mean / rstd the forward stored.  GroupNorm through both output layouts (planes: ocpg_groupnorm_cl_*,
    channels-last: the cl2cl pair).  The launch geometry the bound assumes (workgroups, slots, tiled or not) is asserted against the library.
(b) Dropout: the keep mask is taken from the generator with the probe of test_fused_dropout_add_layernorm and is an input of the reference.
(c) One case per kernel through the autograd bindings (LayerNormLP, fused_ln_func.dropout_add_layer_norm, groupnorm_func.GroupNorm):
    the bindings' fp32 sum of the partials under the same bound, its chain added.
(d) Refused shapes at the ABI: return codes only, and nothing is written.

The `_ex` ports of fused_ln.hip are not re-tested here: tests/test_fused_ln_ports_gpu.py asserts their bit-equality with these kernels.
The worst measured ratios are in DESIGN.md section 4.8b.
"""
import pytest
import torch

import norm_ref as nr

pytestmark = pytest.mark.gpu

LN_CODE = {torch.float32: 1, torch.bfloat16: 0, torch.float16: 2}       # layernorm.hip, groupnorm.hip
DAL_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # fused_ln.hip
RNG = (20240611, 5)
PAIRS = [(c, dt) for c in nr.CASES for dt in nr.DTYPES[c.op]]
PAIR_IDS = ["%s-%s" % (c.name, nr.dtype_id(dt)) for c, dt in PAIRS]
_KEEP = {}


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _keep(case, dev):
    """(b): the mask of RNG on [r, c], from the generator itself; None without dropout"""
    if case.p == 0:
        return None
    if case.name not in _KEEP:
        from test_model_gpu import _probe_keep_mask
        keep = _probe_keep_mask(case.r, case.c, case.p, RNG, dev).float().reshape(case.r, case.c)
        kv = nr.keep_value(case.p)
        assert bool(((keep == 0) | (keep == kv)).all()), "the probe returned something other than 0 or 1/(1-p)"
        if case.r * case.c >= 1000:
            assert abs((keep > 0).float().mean().item() - (1 - case.p)) < 0.03
        _KEEP[case.name] = keep
    return _KEEP[case.name]


def _abi_ln(dev, case, dtype, d):
    from ocpg_amd._lib import lib
    xdt, ydt, gdt, dxdt = nr.io_dtypes("ln", dtype)
    r, c = case.r, case.c
    geo = nr.case_geometry(case)
    nb = lib().ocpg_layernorm_blocks(r)
    assert nb == geo["blocks"], "the bound's geometry assumes the default cap of workgroups"
    y, mean, rstd = _nan((r, c), ydt, dev), _nan((r,), torch.float32, dev), _nan((r,), torch.float32, dev)
    rc = lib().ocpg_layernorm_fwd(d["x"].data_ptr(), LN_CODE[xdt], d["gamma"].data_ptr(), d["beta"].data_ptr(), r, c, nr.EPS, y.data_ptr(),
                                  LN_CODE[ydt], mean.data_ptr(), rstd.data_ptr(), _st())
    assert rc == 0, rc
    dx, part = _nan((r, c), dxdt, dev), _nan((2, nb, c), torch.float32, dev)
    rc = lib().ocpg_layernorm_bwd(d["g"].data_ptr(), LN_CODE[gdt], d["x"].data_ptr(), LN_CODE[xdt], d["gamma"].data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), r, c, dx.data_ptr(), LN_CODE[dxdt], part[0].data_ptr(), part[1].data_ptr(), _st())
    assert rc == 0, rc
    sums = part.double().sum(1)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=sums[0], dbeta=sums[1])


def _abi_dal(dev, case, dtype, d):
    from ocpg_amd._lib import lib
    r, c = case.r, case.c
    geo = nr.case_geometry(case)
    slots = lib().ocpg_dropout_add_ln_bwd_slots(r)
    assert slots == geo["blocks"]
    y, mean, rstd = _nan((r, c), torch.float32, dev), _nan((r,), torch.float32, dev), _nan((r,), torch.float32, dev)
    rc = lib().ocpg_dropout_add_ln_fwd(d["x"].data_ptr(), d["res"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), r, c, nr.EPS, case.p,
                                       RNG[0], RNG[1], None, DAL_CODE[dtype], y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _st())
    assert rc == 0, rc
    gx, gres, part = _nan((r, c), dtype, dev), _nan((r, c), torch.float32, dev), _nan((slots, 2, c), torch.float32, dev)
    rc = lib().ocpg_dropout_add_ln_bwd(d["g"].data_ptr(), d["x"].data_ptr(), d["res"].data_ptr(), d["gamma"].data_ptr(), mean.data_ptr(),
                                       rstd.data_ptr(), r, c, case.p, RNG[0], RNG[1], None, DAL_CODE[dtype], gx.data_ptr(), gres.data_ptr(),
                                       part.data_ptr(), _st())
    assert rc == 0, rc
    sums = part.double().sum(0)
    return dict(y=y, mean=mean, rstd=rstd, gx=gx, gres=gres, dgamma=sums[0], dbeta=sums[1])


def _abi_gn(dev, case, dtype, d):
    from ocpg_amd._lib import lib
    n, hw, c, g = case.n, case.hw, case.c, case.c // nr.D
    words = lib().ocpg_groupnorm_cl_work(n, hw, c, g)
    assert (words > 0) == nr.tiled(case), "the bound's geometry assumes the default tile threshold"
    if words:
        assert words == n * nr.case_geometry(case)["tiles"] * 2 * 256
    work = _nan((words,), torch.float32, dev) if words else None
    wp = None if work is None else work.data_ptr()
    fwd, bwd = (lib().ocpg_groupnorm_cl2cl_fwd, lib().ocpg_groupnorm_cl2cl_bwd) if case.cl else (lib().ocpg_groupnorm_cl_fwd, lib().ocpg_groupnorm_cl_bwd)
    y = _nan((n, hw, c) if case.cl else (n, c, hw), torch.float32, dev)
    mean, rstd = _nan((n, g), torch.float32, dev), _nan((n, g), torch.float32, dev)
    rc = fwd(d["x"].data_ptr(), LN_CODE[dtype], d["gamma"].data_ptr(), d["beta"].data_ptr(), n, hw, c, g, nr.EPS, y.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), wp, _st())
    assert rc == 0, rc
    gy = d["g"] if case.cl else d["g"].permute(0, 2, 1).contiguous()
    dx, part = _nan((n, hw, c), dtype, dev), _nan((n, 2, c), torch.float32, dev)
    rc = bwd(gy.data_ptr(), d["x"].data_ptr(), LN_CODE[dtype], d["gamma"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), n, hw, c, g, dx.data_ptr(),
             part.data_ptr(), wp, _st())
    assert rc == 0, rc
    sums = part.double().sum(0)
    return dict(y=y if case.cl else y.permute(0, 2, 1), mean=mean, rstd=rstd, dx=dx, dgamma=sums[0], dbeta=sums[1])


def _report(tag, got, R, B):
    """Worst ratios, printed; for an output over its bound also the element, what came back, the reference and the bound there."""
    res = nr.ratios(got, R, B)
    print("%s: %s" % (tag, nr.fmt(res)))
    for name, worst in res.items():
        if not worst <= 1.0:
            x = got[name].detach().double()
            diff = (x - R[name]).abs()
            r = torch.where(diff == 0, torch.zeros_like(diff), diff / B[name]).nan_to_num(float("inf")).flatten()
            i = int(r.argmax())
            idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), x.shape))
            print("  %s over its bound at %s: got %.9g ref %.9g bound %.3g ratio %.3g" %
                  (name, idx, x.flatten()[i].item(), R[name].flatten()[i].item(), B[name].flatten()[i].item(), r[i].item()))
    return res


@pytest.mark.parametrize("case,dtype", PAIRS, ids=PAIR_IDS)
def test_every_output_within_the_derived_bound(dev, case, dtype):
    d, R, B = nr.prepared(case, dtype, dev, keep=_keep(case, dev))
    got = {"ln": _abi_ln, "dal": _abi_dal, "gn": _abi_gn}[case.op](dev, case, dtype, d)
    assert set(got) == set(nr.OUTPUTS[case.op])
    res = _report("abi %s %s %s" % (nr.path(case), case.name, nr.dtype_id(dtype)), got, R, B)
    assert max(res.values()) <= 1.0, res


WRAPPED = ["ln-c1024-r4101-rowscale", "dal-c256-r4101-plain", "gn-2x256x60-offset", "gn-t1500-ramp"]
WRAPPED_PAIRS = [(nr.by_name(n), dt) for n in WRAPPED for dt in nr.DTYPES[nr.by_name(n).op]]


@pytest.mark.parametrize("case,dtype", WRAPPED_PAIRS, ids=["%s-%s" % (c.name, nr.dtype_id(dt)) for c, dt in WRAPPED_PAIRS])
def test_autograd_bindings_within_the_derived_bound(dev, case, dtype):
    """(c): y and the gradients through the bindings; dgamma / dbeta are the bindings' own fp32 sums of the partials.  The parameters
    are fp32, so the bindings round nothing further."""
    d, R, B = nr.prepared(case, dtype, dev, keep=_keep(case, dev), wrapper=True)
    xdt, ydt, gdt, dxdt = nr.io_dtypes(case.op, dtype)
    w, b = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    x = d["x"].clone().requires_grad_(True)
    if case.op == "ln":
        from ocpg_amd.models.ops.functions.layernorm_func import LayerNormLP
        y = LayerNormLP.apply(x, w, b, nr.EPS, ydt)
        assert y.dtype == ydt
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), d["g"])
        got = dict(y=y, dx=gx, dgamma=gw, dbeta=gb)
    elif case.op == "dal":
        from ocpg_amd.models.ops.functions import fused_ln_func as f
        norm = torch.nn.LayerNorm(case.c, eps=nr.EPS).to(dev)
        norm.weight, norm.bias = torch.nn.Parameter(w), torch.nn.Parameter(b)
        res = d["res"].clone().requires_grad_(True)
        y = f.dropout_add_layer_norm(x, res, norm, case.p, RNG)
        gx, gr, gw, gb = torch.autograd.grad(y, (x, res, norm.weight, norm.bias), d["g"])
        got = dict(y=y, gx=gx, gres=gr, dgamma=gw, dbeta=gb)
    else:
        from ocpg_amd.models.ops.functions.groupnorm_func import GroupNorm, eligible
        h = {60: 6, 1500: 30}[case.hw]
        wd = case.hw // h
        gn = GroupNorm(case.c // nr.D, case.c, eps=nr.EPS).to(dev)
        with torch.no_grad():
            gn.weight.copy_(d["gamma"]), gn.bias.copy_(d["beta"])
        x4 = d["x"].view(case.n, h, wd, case.c).permute(0, 3, 1, 2).requires_grad_(True)
        assert eligible(x4, gn)
        y = gn(x4)
        assert y.dtype == torch.float32 and type(y.grad_fn).__name__ == "GroupNormCLFunctionBackward"
        gx, gw, gb = torch.autograd.grad(y, (x4, gn.weight, gn.bias), d["g"].view(case.n, h, wd, case.c).permute(0, 3, 1, 2))
        cl = lambda t: t.permute(0, 2, 3, 1).reshape(case.n, case.hw, case.c)
        got = dict(y=cl(y), dx=cl(gx), dgamma=gw, dbeta=gb)
    assert got[[k for k in got if k in ("dx", "gx")][0]].dtype == dxdt
    res = _report("binding %s %s %s" % (nr.path(case), case.name, nr.dtype_id(dtype)), got, R, B)
    assert max(res.values()) <= 1.0, res


def test_refused_shapes_launch_nothing(dev):
    """(d): odd C, C = 260 (no chunk width divides it within 64 lanes) and C = 1040 at ocpg_layernorm_fwd; C = 2052 and C % 4 != 0 at
    ocpg_dropout_add_ln_fwd; groups that are not 8 channels wide at groupnorm_func.eligible.  The output buffers keep their NaN."""
    from ocpg_amd._lib import lib
    from ocpg_amd.models.ops.functions.groupnorm_func import GroupNorm, eligible
    r = 3
    for c in (3, 260, 1040):
        x, gamma, beta = torch.ones(r, c, device=dev), torch.ones(c, device=dev), torch.zeros(c, device=dev)
        y, mean, rstd = _nan((r, c), torch.float32, dev), _nan((r,), torch.float32, dev), _nan((r,), torch.float32, dev)
        rc = lib().ocpg_layernorm_fwd(x.data_ptr(), 1, gamma.data_ptr(), beta.data_ptr(), r, c, nr.EPS, y.data_ptr(), 1, mean.data_ptr(), rstd.data_ptr(), _st())
        assert rc == -2000, (c, rc)
        dx, part = _nan((r, c), torch.float32, dev), _nan((2, 1, c), torch.float32, dev)
        rc = lib().ocpg_layernorm_bwd(x.data_ptr(), 1, x.data_ptr(), 1, gamma.data_ptr(), beta.data_ptr(), beta.data_ptr(), r, c, dx.data_ptr(), 1,
                                      part[0].data_ptr(), part[1].data_ptr(), _st())
        assert rc == -2000, (c, rc)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (y, mean, rstd, dx, part)), c
    for c in (2052, 6, 2):
        x, gamma, beta = torch.ones(r, c, device=dev), torch.ones(c, device=dev), torch.zeros(c, device=dev)
        y, mean, rstd = _nan((r, c), torch.float32, dev), _nan((r,), torch.float32, dev), _nan((r,), torch.float32, dev)
        rc = lib().ocpg_dropout_add_ln_fwd(x.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), r, c, nr.EPS, 0.0, RNG[0], RNG[1], None, 0,
                                           y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _st())
        assert rc == -1006, (c, rc)
        gx, part = _nan((r, c), torch.float32, dev), _nan((1, 2, c), torch.float32, dev)
        rc = lib().ocpg_dropout_add_ln_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), beta.data_ptr(), r, c, 0.0,
                                           RNG[0], RNG[1], None, 0, gx.data_ptr(), None, part.data_ptr(), _st())
        assert rc == -1006, (c, rc)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (y, mean, rstd, gx, part)), c
    x = torch.randn(2, 64, 4, 5, device=dev).contiguous(memory_format=torch.channels_last)
    assert eligible(x, GroupNorm(8, 64).to(dev))
    assert not eligible(x, torch.nn.GroupNorm(16, 64).to(dev)) and not eligible(x, torch.nn.GroupNorm(4, 64).to(dev))
    assert not eligible(x.contiguous(), GroupNorm(8, 64).to(dev))
    # the ABI itself: C != 8 G
    y, st = _nan((2, 64, 20), torch.float32, dev), _nan((2, 2, 16), torch.float32, dev)
    gamma, beta = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    rc = lib().ocpg_groupnorm_cl_fwd(x.data_ptr(), 1, gamma.data_ptr(), beta.data_ptr(), 2, 20, 64, 16, nr.EPS, y.data_ptr(), st[0].data_ptr(),
                                     st[1].data_ptr(), None, _st())
    assert rc == -2000, rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(st).all())
