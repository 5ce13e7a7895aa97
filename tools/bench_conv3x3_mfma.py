"""Micro-benchmark: csrc/conv3x3_mfma.hip (fwd + BN/ReLU epilogue; bwd = bn_act_bwd + MFMA dgrad + im2col/GEMM wgrad) against
MIOpen's conv + the frozen-BN kernel, at the ResNet-101 3x3 shapes of BASELINE config #2 (10 frames, channels-last).
--dtype bf16 (default) | fp16: the storage type of that comparison.
--kernels: instead, one JSON line per own kernel (forward, own-weight input gradient with the mask / scale epilogue -- at stride 2 both
the nine-tap walk, dgrad_w, and the parity-class tiles, dgrad_w_s2 --, weight gradient)
through the C ABI (the _h16 entry points) at every 3x3 site shape of ResNet-101 at 2 clips (20 frames), HIP events around the call, median
of 30, warm (back to back) and cold (1 GiB written between calls), each shape as bf16, fp16, bf16 ("rep" 0 / 1): the two bf16 figures of
one call are the run-to-run spread the fp16 figure is read against."""
import argparse
import json
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ocpg_amd.models import amp_cache, backbone
from ocpg_amd.models.ops.functions import conv_bn_func as f

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
ap.add_argument("--kernels", action="store_true")
ARGS = ap.parse_args()
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[ARGS.dtype]


def kernel_lines():
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    cold_buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)

    def timed(fn, cold, n=30):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            if cold:
                cold_buf.fill_(1.0)
            a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return round(sorted(a.elapsed_time(b) * 1e3 for a, b in ev)[n // 2], 1)

    # (frames, channels, H, W, stride) of conv2 in layer2 / 3 / 4: the stride-2 first block, then the stride-1 blocks
    for (n, c, h, w, s) in ((20, 128, 96, 160, 2), (20, 128, 48, 80, 1), (20, 256, 48, 80, 2), (20, 256, 24, 40, 1), (20, 512, 24, 40, 2),
                            (20, 512, 12, 20, 1)):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        for dname, code, rep in (("bf16", 1, 0), ("fp16", 2, 0), ("bf16", 1, 1)):
            tdt = torch.bfloat16 if code == 1 else torch.float16
            g = torch.Generator().manual_seed(0)
            x = torch.randn(n, h, w, c, generator=g).to(dev, tdt)
            wt = (torch.randn(c, 3, 3, c, generator=g) * 0.02).to(dev, tdt)
            gz = torch.randn(n, ho, wo, c, generator=g).to(dev, tdt)
            scale, shift = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
            y, dx = torch.empty(n, ho, wo, c, dtype=tdt, device=dev), torch.empty(n, h, w, c, dtype=tdt, device=dev)
            sp = int(L.ocpg_conv3x3_mfma_wgrad_splits(n, h, w, c, c, s))
            part = torch.empty(sp, c, 9 * c, dtype=tdt, device=dev)

            def fwd():
                assert L.ocpg_conv3x3_mfma_fwd_cols_h16(x.data_ptr(), wt.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, n, h, w, c, c, s,
                                                        y.data_ptr(), None, code, st) == 0

            def dgrad():
                assert L.ocpg_conv3x3_mfma_dgrad_w_h16(gz.data_ptr(), wt.data_ptr(), x.data_ptr(), scale.data_ptr(), n, h, w, c, c, s, dx.data_ptr(),
                                                       code, st) == 0

            def wgrad():
                assert L.ocpg_conv3x3_mfma_wgrad_h16(gz.data_ptr(), x.data_ptr(), n, h, w, c, c, s, part.data_ptr(), code, st) == 0

            def dgrad_s2():     # stride 2 only: the same input gradient in parity-class tiles (what the step runs by default)
                assert L.ocpg_conv3x3_mfma_dgrad_w_s2_h16(gz.data_ptr(), wt.data_ptr(), x.data_ptr(), scale.data_ptr(), n, h, w, c, c, s, dx.data_ptr(),
                                                          code, st) == 0

            for name, fn in (("fwd", fwd), ("dgrad_w", dgrad)) + ((("dgrad_w_s2", dgrad_s2),) if s == 2 else ()) + (("wgrad", wgrad),):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                warm, cold = timed(fn, False), timed(fn, True)
                print(json.dumps({"kernel": name, "dtype": dname, "rep": rep, "frames": n, "C": c, "H": h, "W": w, "stride": s,
                                  "warm_us": warm, "cold_us": cold, "TFLOPs_warm": round(2.0 * n * ho * wo * c * c * 9 / warm / 1e6, 1)}), flush=True)


if ARGS.kernels:
    kernel_lines()
    sys.exit(0)


def timeit(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


for (n, c, h, w, s) in ((10, 128, 48, 80, 1), (10, 256, 24, 40, 1), (10, 512, 12, 20, 1), (10, 256, 48, 80, 2), (10, 512, 24, 40, 2)):
    x = torch.randn(n, c, h, w, device=dev).to(DT).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wt = (torch.randn(c, c, 3, 3, device=dev) * 0.02).to(DT).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    scale, shift = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    go = torch.randn(n, c, ho, wo, device=dev).to(DT).contiguous(memory_format=torch.channels_last)
    flops = 2.0 * n * ho * wo * c * c * 9

    def mfma_f():
        return f.conv3x3_mfma_bn_act(x, wt, scale, shift, True, s, 1)

    def mfma_fb():
        torch.autograd.grad(mfma_f(), (x, wt), go)

    def mio_f():
        y = torch.nn.functional.conv2d(x, wt, None, s, 1)
        return backbone.bn_act_func.frozen_bn_act(y, scale, shift, None, True) if hasattr(backbone, "bn_act_func") else (y * scale.view(1, -1, 1, 1).to(y.dtype) + shift.view(1, -1, 1, 1).to(y.dtype)).relu()

    def mio_fb():
        torch.autograd.grad(mio_f(), (x, wt), go)
    with torch.no_grad():
        tf_m, tf_o = timeit(mfma_f), timeit(mio_f)
    tb_m, tb_o = timeit(mfma_fb), timeit(mio_fb)
    print(f"{c:4d}ch {h}x{w}/s{s}: fwd mfma {tf_m:7.1f} us ({flops / tf_m / 1e6:6.1f} TFLOP/s)  miopen+bn {tf_o:7.1f} us | "
          f"fwd+bwd mfma {tb_m:7.1f} us  miopen+bn {tb_o:7.1f} us", flush=True)
