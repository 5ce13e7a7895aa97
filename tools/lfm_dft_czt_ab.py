"""Three-way A/B of the LFM block on maps with a prime side 67..127: the library route (rocFFT between the transposing kernels), the direct
O(p^2) stage of csrc/lfm_dft_any.hip (modules.DFT_ANY_MAX_PRIME lifted) and the chirp-z line transform of csrc/lfm_dft_czt.hip.  The
conditions of tools/lfm_dft_any_ab.py: one GPU, one process, the legs alternated call by call, each call between its own pair of device
events, operands cold (a buffer larger than L2 + MALL is rewritten before every timed call, outside the events), medians of --iters calls,
and the library leg run twice: the distance of its two medians is the spread a difference has to exceed.

One LFMResizeAdaptive(256, 7), forward + backward, bf16 autocast as in training, on 36 x 60 x 107 and 16 x 60 x 107 (what unpadded 480 x 854
frames leave at stride 8) and on 10 x 40 x p and 10 x p x 40 for every prime 67 <= p <= 127.  The input is in the memory GroupNorm hands over
at such a size (planes, NCHW), so the own routes pay one channels-last copy; "chirp_nhwc_input" is the chirp route fed channels-last memory.

modules.DFT_CZT_MIN_PRIME follows from the sweep lines: the smallest prime from which the chirp leg beats BOTH other legs on BOTH axes by more
than the spread, at that prime and every larger one ("czt_min_prime" in the last line; null when no prime qualifies).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import statistics

sys.path.insert(0, ROOT)
import torch

from ocpg_amd import _lib
from ocpg_amd.models import fallbacks, modules
from ocpg_amd.models.ops.functions import spectral_func as sf

C = 256
EVAL = [(36, 60, 107), (16, 60, 107)]
PRIMES = [67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127]
# leg -> (DFT_CZT, DFT_CZT_FORCE, DFT_ANY_MAX_PRIME): the library leg also keeps the primes 67..79 away from the direct stage
LEGS = {"library": (False, False, 16), "direct": (False, False, 127), "chirp": (True, True, 79)}


def timed(fns, iters, before=None):
    """Alternate the callables; -> per-callable list of per-call milliseconds."""
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "calls": len(ms)}


def set_leg(name):
    modules.DFT_CZT, modules.DFT_CZT_FORCE, modules.DFT_ANY_MAX_PRIME = LEGS[name]


def block_ab(dev, iters, emit, groups):
    torch.manual_seed(0)
    lfm = modules.LFMResizeAdaptive(C, 7).to(dev)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)       # 1 GiB: past the 256 MB MALL

    def cold():
        flush.add_(1)

    saved = (modules.DFT_CZT, modules.DFT_CZT_FORCE, modules.DFT_ANY_MAX_PRIME)
    lines = []
    try:
        for kind, shapes in groups:
            for n, h, w in shapes:
                planes = torch.randn(n, C, h, w, device=dev)
                nhwc = planes.contiguous(memory_format=torch.channels_last)
                go = torch.randn(n, C, h, w, device=dev)

                def run(leg, src, keep=False):
                    set_leg(leg)
                    x = src.detach().requires_grad_(True)
                    lfm.zero_grad(set_to_none=True)
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        y, _ = lfm(x)
                    y.backward(go)
                    return (y.detach(), x.grad) if keep else None

                outs, counts = {}, {}
                for leg in LEGS:
                    fallbacks.reset()
                    calls = _lib.census(True)
                    outs[leg] = run(leg, planes, True)
                    _lib.census(False)
                    counts[leg] = {k: v for k, v in calls.items() if k.startswith("ocpg_lfm_spectrum")}
                    counts[leg]["library_fallbacks"] = sum(v for k, v in fallbacks.snapshot().items() if k.startswith("LFM"))
                assert set(counts["chirp"]) == {"ocpg_lfm_spectrum_fwd_czt", "ocpg_lfm_spectrum_inv_czt", "library_fallbacks"}, counts
                assert set(counts["direct"]) == {"ocpg_lfm_spectrum_fwd_any", "ocpg_lfm_spectrum_inv_any", "library_fallbacks"}, counts
                assert counts["library"] == {"library_fallbacks": 1}, counts
                diff = {"out_max_abs": outs["library"][0].abs().max().item(), "gx_max_abs": outs["library"][1].abs().max().item()}
                for leg in ("direct", "chirp"):
                    diff[f"{leg}_out_max_abs_diff"] = (outs[leg][0] - outs["library"][0]).abs().max().item()
                    diff[f"{leg}_gx_max_abs_diff"] = (outs[leg][1] - outs["library"][1]).abs().max().item()
                del outs
                fns = [lambda: run("library", planes), lambda: run("direct", planes), lambda: run("chirp", planes), lambda: run("library", planes),
                       lambda: run("chirp", nhwc)]
                for fn in fns:
                    for _ in range(3):
                        fn()
                res = [stats(m) for m in timed(fns, iters, cold)]
                lib_, direct, chirp = res[0]["median_ms"], res[1]["median_ms"], res[2]["median_ms"]
                spread = abs(res[0]["median_ms"] - res[3]["median_ms"]) / res[0]["median_ms"]
                line = {"part": "block", "kind": kind, "N": n, "C": C, "h": h, "w": w, "chirp_axes": [modules._is_prime(h) and h >= 67, modules._is_prime(w) and w >= 67],
                        "library": res[0], "direct": res[1], "chirp": res[2], "library_again": res[3], "chirp_nhwc_input": res[4],
                        "library_over_chirp_median": round(lib_ / chirp, 3), "direct_over_chirp_median": round(direct / chirp, 3),
                        "library_over_direct_median": round(lib_ / direct, 3), "identical_runs_spread": round(spread, 4),
                        "chirp_beats_both_by_more_than_spread": bool(chirp * (1 + spread) < min(lib_, direct)), "entry_points": counts, **diff}
                lines.append(line)
                emit(line)
    finally:
        modules.DFT_CZT, modules.DFT_CZT_FORCE, modules.DFT_ANY_MAX_PRIME = saved
        fallbacks.reset()
    return lines


def min_prime(lines):
    """The smallest prime from which every sweep line (both axes), at that prime and every larger one, has the chirp leg ahead of both others."""
    wins = {p: all(ln["chirp_beats_both_by_more_than_spread"] for ln in lines if ln["kind"].startswith("sweep") and p in (ln["h"], ln["w"])) for p in PRIMES}
    best = None
    for p in reversed(PRIMES):
        if not wins[p]:
            break
        best = p
    return best, wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfm_dft_czt_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lfm_dft_czt_ab: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)             # the library leg is a counted fallback: that is what it measures
    with open(a.out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        lines = block_ab(dev, a.iters, emit, (("eval", EVAL), ("sweep_w", [(10, 40, p) for p in PRIMES]), ("sweep_h", [(10, p, 40) for p in PRIMES])))
        best, wins = min_prime(lines)
        emit({"part": "default", "czt_min_prime": best, "chirp_beats_both_on_both_axes": {str(p): w for p, w in wins.items()},
              "channels_per_workgroup": sf.CZT_SLAB})


if __name__ == "__main__":
    main()
