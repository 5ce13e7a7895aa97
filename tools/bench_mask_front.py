"""The mask head's front end on its own, at the bench shape (2 clips of 5 x 384 x 640, C = 256): the torch lines between the transformer's
return and the criterion (memory fusion; level-set feature stack) and the memory fusion by csrc/mask_front.hip, one eager forward +
backward each under torch.profiler (launches, summed kernel time); then every mask_front kernel with HIP events on cold operands (1 GiB
written between calls), its algorithmic bytes against 8 TB/s."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from torch.profiler import profile, ProfilerActivity
from ocpg_amd.models.resample import bicubic_resize, bilinear_resize

dev = torch.device("cuda:0")
torch.manual_seed(0)
B, T, C = 2, 5, 256
N = B * T
shapes = [(48, 80), (24, 40), (12, 20), (6, 10)]
S = sum(h * w for h, w in shapes)
H, W = 384, 640


def kernels(prof):
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(ev), sum(e.device_time_total for e in ev)


def report(tag, fn, reps=3):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    n, us = kernels(prof)
    print("%-34s %5.1f launches  %8.1f us per call" % (tag, n / reps, us / reps), flush=True)
    agg = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            a = agg.setdefault(e.name[:90], [0, 0.0])
            a[0] += 1
            a[1] += e.device_time_total
    for k, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:14]:
        print("      %5.1f x %8.1f us  %s" % (c / reps, t / reps, k))


# ---- memory fusion: slices + permute copies + bicubic matmuls + the channels-last copy _ls_feat makes, forward and backward
mem = torch.randn(N, S, C, device=dev, requires_grad=True)
g_nchw = torch.randn(N, C, 48, 80, device=dev)
g_cl = torch.randn(N, 48, 80, C, device=dev)


def memfuse_torch():
    feats, start = [], 0
    for (h, w) in shapes[:3]:
        feats.append(mem[:, start:start + h * w].reshape(N, h, w, C).permute(0, 3, 1, 2).contiguous())
        start += h * w
    tar = feats[0].shape[-2:]
    fusion = sum(bicubic_resize(x.float(), tar) for x in feats)
    cl = fusion.permute(0, 2, 3, 1).contiguous()
    return torch.autograd.grad([fusion, cl], [mem], [g_nchw, g_cl])


report("memfuse torch fwd+bwd", memfuse_torch)

# ---- level-set feature stack
lsf0 = torch.randn(N, 48, 80, 8, device=dev).permute(0, 3, 1, 2).to(torch.bfloat16).requires_grad_(True)
txt0 = torch.randn(B, 8, device=dev, requires_grad=True)
frames = torch.randn(N, 3, H, W, device=dev)
g11 = torch.randn(B, T, 11, 192, 320, device=dev)


def lsfeat_torch(lsf_in=lsf0):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lsf = lsf_in
        ls_feat = bilinear_resize(lsf, (4 * lsf.shape[-2], 4 * lsf.shape[-1]), True).unflatten(0, (B, T))
        txt = txt0[:, None, :, None, None]
        sim = (ls_feat * txt).sum(dim=2) / ((F.normalize(ls_feat, dim=2) * F.normalize(txt, dim=2)).sum(dim=2) + 1e-5)
        img = bilinear_resize(frames, tuple(ls_feat.shape[-2:]), True).unflatten(0, (B, T))
        ls_features = torch.cat([img, ls_feat, sim.unsqueeze(2)], dim=2)
    return torch.autograd.grad([ls_features[:, :, :-1]], [lsf_in, txt0], [g11], allow_unused=True)


report("lsfeat torch fwd+bwd (bf16 lsf)", lsfeat_torch)

if os.environ.get("TORCH_ONLY") != "1":      # TORCH_ONLY=1: a tree without the kernels (the parent)
    from ocpg_amd.models.ops.functions.mask_front_func import memfuse
    hw = tuple(shapes)

    def memfuse_hip():
        nchw, cl = memfuse(mem, hw, 3, True, True)
        return torch.autograd.grad([nchw, cl], [mem], [g_nchw, g_cl])

    report("memfuse HIP fwd+bwd", memfuse_hip)
    a, b = memfuse_torch()[0], memfuse_hip()[0]
    print("memfuse grad max |torch - hip| = %.3e of max %.3e" % ((a - b).abs().max().item(), a.abs().max().item()))

    from ocpg_amd.models.ops.functions.mask_front_func import lsfeat

    def lsfeat_hip():
        out = lsfeat(lsf0, txt0, frames, B, T, (192, 320))
        return torch.autograd.grad([out[:, :, :-1]], [lsf0, txt0], [g11])

    report("lsfeat HIP fwd+bwd (bf16 lsf)", lsfeat_hip)

    # cold-operand timing: 1 GiB written between calls
    import ctypes
    from ocpg_amd._lib import lib
    from ocpg_amd.models.ops.functions import mask_front_func as mf
    big = torch.empty(1 << 28, device=dev)
    wts, rng, geom = mf.tables(hw, 3, dev)
    o_nchw, o_cl, gm = torch.empty_like(g_nchw), torch.empty_like(g_cl), torch.empty_like(mem)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = lib()
    md = mem.detach()
    used = sum(h * w for h, w in shapes[:3]) * N * C * 4
    port = g_nchw.numel() * 4

    def f(a, b):
        return lambda: L.ocpg_memfuse_fwd_f32(md.data_ptr(), wts.data_ptr(), rng.data_ptr(), geom.data_ptr(), wts.numel(), rng.numel(), 4, 3, N, S, C,
                                              a, b, st)

    def bw(a, b):
        return lambda: L.ocpg_memfuse_bwd_f32(a, b, wts.data_ptr(), rng.data_ptr(), geom.data_ptr(), wts.numel(), rng.numel(), 4, 3, N, S, C,
                                              gm.data_ptr(), st)
    cases = [("fwd both ports", f(o_nchw.data_ptr(), o_cl.data_ptr()), used + 2 * port),
             ("fwd nchw only", f(o_nchw.data_ptr(), None), used + port),
             ("bwd both gradients", bw(g_nchw.data_ptr(), g_cl.data_ptr()), 2 * port + mem.numel() * 4),
             ("bwd nchw only", bw(g_nchw.data_ptr(), None), port + mem.numel() * 4)]
    tab_i, tab_w, off = mf.ls_tables(48, 80, H, W, 192, 320, dev)
    lcl = lsf0.detach().permute(0, 2, 3, 1).contiguous()
    lo, gl, gp = torch.empty(B, T, 12, 192, 320, device=dev), torch.empty(N, 48, 80, 8, device=dev), torch.empty(B, L.ocpg_lsfeat_bwd_parts(T, 192, 320), 8, device=dev)
    gfull = torch.randn(B, T, 12, 192, 320, device=dev)
    gzero = gfull.clone()
    gzero[:, :, 11] = 0
    tx = txt0.detach()

    def lb(gg):
        return lambda: L.ocpg_lsfeat_bwd_f32(gg.data_ptr(), lcl.data_ptr(), 1, tx.data_ptr(), tab_i.data_ptr(), tab_w.data_ptr(), off.data_ptr(), B, T,
                                             48, 80, 192, 320, gl.data_ptr(), gp.data_ptr(), st)
    cases += [("lsfeat fwd", lambda: L.ocpg_lsfeat_fwd_f32(lcl.data_ptr(), 1, tx.data_ptr(), frames.data_ptr(), tab_i.data_ptr(), tab_w.data_ptr(),
                                                           off.data_ptr(), B, T, 48, 80, H, W, 192, 320, lo.data_ptr(), st),
               lo.numel() * 4 + frames.numel() * 4 + lcl.numel() * 2),
              ("lsfeat bwd, g[11] = 0", lb(gzero), gfull.numel() * 4 * 9 // 12 + gl.numel() * 4),
              ("lsfeat bwd, g[11] != 0", lb(gfull), gfull.numel() * 4 * 9 // 12 + gl.numel() * 4)]
    for name, call, nbytes in cases:
        ts = []
        for _ in range(5):
            big.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); rc = call(); e1.record(); torch.cuda.synchronize()
            assert rc == 0, rc
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        print("cold %-20s median %7.1f us  min %7.1f us  %6.1f MB  -> %5.2f TB/s at the median (%.1f us at 8 TB/s)"
              % (name, ts[2], ts[0], nbytes / 1e6, nbytes / ts[2] / 1e6, nbytes / 8e6))
