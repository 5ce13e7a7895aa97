"""conv3x3_mfma without the work a step does not use, the part that needs no GPU: the compiler's own resource remarks for
csrc/conv3x3_mfma.hip (tools/kernel_resource_usage.py).  No instantiation of the kernel may use scratch (the bf16 64-column epilogue did,
through a run-time index into its output registers), the forward without the patch-matrix output (COLS = false, the shipped step's) must
fit three workgroups per CU (a workgroup is four waves: occupancy 3 waves per SIMD), and the patch-matrix output must still exist as its
own instantiation (COLS = true, behind OCPG_CONV3X3_FWD_COLS)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kernels():
    from ocpg_amd.csrc import build
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip("hipcc is not installed")
    import kernel_resource_usage
    ks = kernel_resource_usage.compile_remarks(["conv3x3_mfma.hip"])
    return {k: v for k, v in ks.items() if k.startswith("conv3x3_mfma<") or k.startswith("conv3x3_mfma_f16<")}


def test_no_instantiation_uses_scratch(kernels):
    assert len(kernels) >= 13, sorted(kernels)
    assert {k.split("<")[0] for k in kernels} == {"conv3x3_mfma", "conv3x3_mfma_f16"}
    bad = {k: v["ScratchSize [bytes/lane]"] for k, v in kernels.items() if v["ScratchSize [bytes/lane]"] != 0}
    assert not bad, bad


@pytest.mark.parametrize("name", ["conv3x3_mfma", "conv3x3_mfma_f16"])
def test_forward_without_cols_fits_three_workgroups_per_cu(kernels, name):
    k = kernels[name + "<false, 64, false, false, false, false>"]
    print(name, k)
    assert k["Occupancy [waves/SIMD]"] == 3, k


def test_cols_instantiations_exist(kernels):
    for name in ("conv3x3_mfma", "conv3x3_mfma_f16"):
        for bn in (64, 128):
            assert name + "<false, %d, false, false, true, false>" % bn in kernels, sorted(kernels)


def test_parity_class_instantiations_exist(kernels):
    for name in ("conv3x3_mfma", "conv3x3_mfma_f16"):
        for bn in (64, 128):
            assert name + "<true, %d, false, true, false, true>" % bn in kernels, sorted(kernels)
