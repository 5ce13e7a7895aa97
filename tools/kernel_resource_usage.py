"""Kernel resource usage (registers, scratch, occupancy, static LDS) of the kernels of csrc/*.hip, from the compiler's own remarks
(hipcc -Rpass-analysis=kernel-resource-usage; needs no GPU).  One line per kernel, sorted by name, so that two listings diff cleanly:

    python tools/kernel_resource_usage.py 'msda*.hip' > profiles/msda_resource_usage.txt
    python tools/kernel_resource_usage.py bn_act.hip conv3x3_mfma.hip conv3x3_wgrad.hip gemm_dgrad_bn.hip

Arguments are file patterns relative to ocpg_amd/csrc (default: every source); `--remarks FILE...` parses saved remark files instead of
compiling.  The lines of existing kernels must not move when a kernel next to them is added or templated (DESIGN.md sections 4.3b, 4.9)."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocpg_amd.csrc import build  # noqa: E402

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def parse(text):
    """remarks of one compile -> {demangled kernel name: {field: value}}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:.*?)Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for f in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(f) + r": (\d+)", line)
            if m:
                cur[f] = int(m.group(1))
    if not out:
        return {}
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return {d.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0]: out[n] for n, d in zip(names, dem)}


def listing(kernels):
    rows = []
    for name in sorted(kernels):
        k = kernels[name]
        rows.append("%-78s sgpr %3d  vgpr %3d  agpr %3d  scratch %4d  occupancy %d  lds %6d" % (
            name, k.get("TotalSGPRs", -1), k.get("VGPRs", -1), k.get("AGPRs", -1), k.get("ScratchSize [bytes/lane]", -1),
            k.get("Occupancy [waves/SIMD]", -1), k.get("LDS Size [bytes/block]", -1)))
    return "\n".join(rows)


def compile_remarks(patterns):
    """{kernel: fields} of every source under csrc/ that matches one of the patterns"""
    srcs = sorted({s for p in patterns for s in glob.glob(os.path.join(build.HERE, p))})
    if not srcs:
        raise SystemExit("no source matches %s under %s" % (" ".join(patterns), build.HERE))
    kernels = {}
    for src in srcs:
        cmd = [build.HIPCC] + build.CFLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
        kernels.update(parse(subprocess.run(cmd, capture_output=True, text=True, check=True).stderr))
    return kernels


def main(argv, default_patterns=("*.hip",)):
    if argv and argv[0] == "--remarks":
        kernels = {}
        for p in argv[1:]:
            kernels.update(parse(open(p).read()))
    else:
        kernels = compile_remarks(argv or list(default_patterns))
    print(listing(kernels))


if __name__ == "__main__":
    main(sys.argv[1:])
