"""The 1x1 input gradient with the frozen-BN + ReLU backward of the layer in front in its epilogue (csrc/gemm_dgrad_bn.hip,
conv_bn_func.FUSED_DGRAD_BN): the kernel against an fp32 matmul of the same bf16 inputs at the ResNet-101 body's site shapes, a chain of
bottlenecks with the switch on and off, and the guard against a second consumer of a fused intermediate."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M at 2 clips of 10 frames, N = Cin of the 1x1 conv, K = its Cout): site (a) conv3's input gradient, site (b) conv1's
SITES = {"a_L2": (38400, 128, 512), "a_L3": (9600, 256, 1024), "a_L4": (2400, 512, 2048),
         "b_L2": (38400, 512, 128), "b_L3": (9600, 1024, 256), "b_L4": (2400, 2048, 512)}
CASES = [(name, m // b, n, k) for name, (m, n, k) in SITES.items() for b in (1, 2)] + [("ragged", 333, 256, 384), ("small", 1, 128, 128)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _call(a, w, c, mask, scale, out, out_skip, tile=None):
    from ocpg_amd._lib import lib, stream_ptr
    L = lib()
    m, k = a.shape
    n = w.shape[1]
    t = int(L.ocpg_gemm_dgrad_bn_tile(m, n, k)) if tile is None else tile
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    return L.ocpg_gemm_dgrad_bn(p(a), p(w), p(c), p(mask), p(scale), p(out), p(out_skip), m, n, k, 1, t, stream_ptr())


def _ulps(x, ref):
    """|x - ref| in units of the bf16 spacing at |ref| (ref rounded to bf16 first)."""
    r = ref.to(torch.bfloat16).float()
    spacing = torch.where(r == 0, torch.full_like(r, 2.0 ** -133), 2.0 ** (torch.floor(torch.log2(r.abs())) - 7))
    return ((x.float() - r).abs() / spacing)


@pytest.mark.parametrize("mode", ["a", "b", "plain"])
@pytest.mark.parametrize("name,m,n,k", CASES)
def test_kernel_against_fp32(dev, mode, name, m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev, torch.bfloat16)
    mask = torch.randn(m, n, generator=g).to(dev, torch.bfloat16)
    scale = (torch.rand(n, generator=g) + 0.5).to(dev)
    c = torch.randn(m, n, generator=g).to(dev, torch.bfloat16)
    v = a.float() @ w.float()
    out = torch.empty(m, n, dtype=torch.bfloat16, device=dev)
    if mode == "a":
        assert _call(a, w, None, mask, scale, out, None) == 0
        refs = [(out, torch.where(mask.float() > 0, v, torch.zeros_like(v)) * scale)]
    elif mode == "b":
        c0 = c.clone()
        assert _call(a, w, c, mask, scale, out, c) == 0                 # out_skip over C, in place
        mm = torch.where(mask.float() > 0, v + c0.float(), torch.zeros_like(v))
        refs = [(c, mm), (out, mm * scale)]
    else:
        assert _call(a, w, None, None, None, out, None) == 0
        refs = [(out, v)]
    torch.cuda.synchronize()
    for got, ref in refs:
        # fp32 accumulation in another order: <= 2 bf16 ulps wherever the sum is not the result of heavy cancellation; all of it within
        # a norm-relative 2^-8, bf16's unit roundoff (the final rounding alone is ~1.1e-3 in norm)
        u = _ulps(got, ref)
        big = ref.abs() > 1e-2 * ref.abs().max()
        assert u[big].max().item() <= 2.0, (name, mode, u[big].max().item())
        assert (got.float() - ref).norm().item() <= 2.0 ** -8 * ref.norm().item() + 1e-6


@pytest.mark.parametrize("name,m,n,k", CASES)
def test_tiles_agree_and_fill_the_chip(dev, name, m, n, k):
    """Every tile computes each element as the same fp32 chain over k: bit-identical results (mode b: C in place, mask, scale).  The
    chosen tile (64 x 64) fills the 256 CUs at every site shape of 2 clips."""
    from ocpg_amd._lib import lib
    sizes = {0: (128, 128), 1: (64, 128), 2: (64, 64)}
    wgs = {t: (m + tm - 1) // tm * (n // tn) for t, (tm, tn) in sizes.items() if n % tn == 0}
    assert int(lib().ocpg_gemm_dgrad_bn_tile(m, n, k)) == 2
    if name in SITES and m == SITES[name][0]:
        assert wgs[2] >= 256, wgs
    g = torch.Generator().manual_seed(3)
    a = torch.randn(m, k, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev, torch.bfloat16)
    mask = torch.randn(m, n, generator=g).to(dev, torch.bfloat16)
    scale = (torch.rand(n, generator=g) + 0.5).to(dev)
    c0 = torch.randn(m, n, generator=g).to(dev, torch.bfloat16)
    res = []
    for tile in sorted(wgs):
        c = c0.clone()
        out = torch.empty(m, n, dtype=torch.bfloat16, device=dev)
        assert _call(a, w, c, mask, scale, out, c, tile=tile) == 0
        res.append((out, c))
    torch.cuda.synchronize()
    for out, c in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(c, res[0][1])


def test_declines(dev):
    """Shapes, alignments and dtypes the kernel does not serve come back as the three decline codes, with nothing written."""
    from ocpg_amd._lib import lib, stream_ptr
    L = lib()
    a = torch.zeros(64, 256, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(256, 256, dtype=torch.bfloat16, device=dev)
    out = torch.full((64, 256), 7.0, dtype=torch.bfloat16, device=dev)
    st = stream_ptr()
    assert L.ocpg_gemm_dgrad_bn(a.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), None, 64, 192, 256, 1, 0, st) == -2000
    assert L.ocpg_gemm_dgrad_bn(a.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), None, 64, 256, 192, 1, 0, st) == -2000
    assert L.ocpg_gemm_dgrad_bn(a.data_ptr() + 2, w.data_ptr(), None, None, None, out.data_ptr(), None, 64, 256, 128, 1, 0, st) == -2001
    assert L.ocpg_gemm_dgrad_bn(a.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), None, 64, 256, 256, 0, 0, st) == -2002
    assert L.ocpg_gemm_dgrad_bn_tile(64, 96, 256) == -1 and L.ocpg_gemm_dgrad_bn_tile(64, 256, 192) == -1
    torch.cuda.synchronize()
    assert bool((out.float() == 7.0).all())


def _chain(dev, width, nblocks):
    from ocpg_amd.models import backbone
    torch.manual_seed(7)
    blocks = [backbone.Bottleneck(width * 2, width, 2, 1, True)] + [backbone.Bottleneck(width * 4, width, 1, 1, False) for _ in range(nblocks - 1)]
    seq = torch.nn.Sequential(*blocks).to(dev)
    for m in seq.modules():
        if isinstance(m, backbone.FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.1), m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 1.5)
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    return seq.to(torch.bfloat16)


def _run(seq, x, go, fused):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func
    old = conv_bn_func.FUSED_DGRAD_BN
    conv_bn_func.FUSED_DGRAD_BN = fused
    try:
        conv_bn_func.reset_skip_tokens()
        xi = x.clone().requires_grad_(True)
        seq.zero_grad()
        calls = _lib.census(True)
        y = seq(xi)
        y.backward(go)
        torch.cuda.synchronize()
        counts = dict(calls)
        _lib.census(False)
        return [y.detach().float(), xi.grad.float()] + [p.grad.float() for p in seq.parameters()], counts
    finally:
        conv_bn_func.FUSED_DGRAD_BN = old


def test_bottleneck_chain_fused_dgrad_bn(dev):
    """A projecting bottleneck and three identity ones at layer3's width and map (10 frames of 24 x 40), bf16 channels-last: forward
    identical with the switch on and off, every gradient within the bound of test_bottleneck_premasked_input_gradient, and the census one
    ocpg_bn_act_bwd less per site: 4 sites (a) (every conv3's input gradient) + 3 sites (b) (the identity blocks' conv1)."""
    seq = _chain(dev, 256, 4)
    x = torch.randn(10, 512, 48, 80, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    go = torch.randn(10, 1024, 24, 40, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    on, c_on = _run(seq, x, go, True)
    off, c_off = _run(seq, x, go, False)
    assert c_on.get("ocpg_gemm_dgrad_bn", 0) == 7 and c_off.get("ocpg_gemm_dgrad_bn", 0) == 0, (c_on, c_off)
    assert c_on.get("ocpg_bn_act_bwd", 0) == c_off.get("ocpg_bn_act_bwd", 0) - 7, (c_on, c_off)
    assert torch.equal(on[0], off[0])
    for a, b_ in zip(on[1:], off[1:]):
        assert (a - b_).norm().item() <= 1e-2 * b_.norm().item(), ((a - b_).norm().item(), b_.norm().item())


def test_second_consumer_of_fused_intermediate_raises(dev):
    """An identity block's input read by a second consumer outside the block: with the switch on the producer's backward refuses the
    gradient (it would be masked and scaled twice); with it off the gradients are those of the same graph without the fusion."""
    seq = _chain(dev, 128, 2)
    x = torch.randn(2, 256, 16, 20, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, 512, 8, 10, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    from ocpg_amd.models.ops.functions import conv_bn_func

    def run(fused):
        old = conv_bn_func.FUSED_DGRAD_BN
        conv_bn_func.FUSED_DGRAD_BN = fused
        try:
            conv_bn_func.reset_skip_tokens()
            xi = x.clone().requires_grad_(True)
            seq.zero_grad()
            mid = seq[0](xi)                 # block 0's conv3 output: the producer of site (b)
            y = seq[1](mid)
            (y.float() * go.float()).sum().add_((mid.float() ** 2).sum() * 1e-3).backward()      # second consumer of mid
            torch.cuda.synchronize()
            return [xi.grad.float()] + [p.grad.float() for p in seq.parameters()]
        finally:
            conv_bn_func.FUSED_DGRAD_BN = old

    with pytest.raises(RuntimeError, match="OCPG_FUSED_DGRAD_BN"):
        run(True)
    got = run(False)
    # the same graph in fp32 on the host (the modules' CPU path: convolution + frozen BN, no fused kernels)
    import copy
    ref_seq = copy.deepcopy(seq).float().cpu()
    xr = x.float().cpu().requires_grad_(True)
    mid = ref_seq[0](xr)
    y = ref_seq[1](mid)
    (y * go.float().cpu()).sum().add_((mid ** 2).sum() * 1e-3).backward()
    ref = [xr.grad] + [p.grad for p in ref_seq.parameters()]
    # bf16 through two blocks against fp32 differs by a few per cent (up to ~6 % seen on a 1x1 weight gradient); a second mask-and-scale
    # of block 0's gradient (scale ~ U(0.5, 1.5) / sqrt(U(0.5, 1.5))) would be off by tens of per cent
    for a, b_ in zip(got, ref):
        a = a.cpu()
        assert (a - b_).norm().item() <= 1e-1 * b_.norm().item(), ((a - b_).norm().item(), b_.norm().item())


def test_second_consumer_of_premasked_intermediate_raises(dev):
    """The same guard on the conv1 -> conv2 pair (OCPG_PREMASK_DGRAD): conv1's output read by a second consumer besides the 3x3 conv2 makes
    conv1's backward refuse the gradient instead of masking and scaling it a second time; with the switch off the backward runs."""
    from ocpg_amd.models import backbone
    from ocpg_amd.models.ops.functions import conv_bn_func
    torch.manual_seed(11)
    blk = backbone.Bottleneck(512, 128, 1, 1, True).to(dev)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    blk = blk.to(torch.bfloat16)
    x = torch.randn(2, 512, 16, 20, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def run(on):
        old = conv_bn_func.PREMASK
        conv_bn_func.PREMASK = on
        try:
            conv_bn_func.reset_skip_tokens()
            xi = x.clone().requires_grad_(True)
            y1 = backbone.conv_bn_act(blk.conv1, blk.bn1, xi, None, True)
            y2 = backbone.conv_bn_act(blk.conv2, blk.bn2, y1, None, True)
            (y2.float().sum() + (y1.float() ** 2).sum() * 1e-3).backward()
            torch.cuda.synchronize()
            return xi.grad
        finally:
            conv_bn_func.PREMASK = old

    with pytest.raises(RuntimeError, match="OCPG_PREMASK_DGRAD"):
        run(True)
    assert torch.isfinite(run(False).float()).all()
