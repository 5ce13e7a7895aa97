"""The FFN epilogue modes of csrc/gemm_dgrad_bn.hip, the part that needs no GPU: the compiler's own resource remarks
(tools/kernel_resource_usage.py).  The new instantiations (gemm_ffn<TM, TN, mode>) use no scratch, and the lines of the existing ones
(gemm_dgrad_bn, gemm_dgrad_bn_f16: the ResNet body's 1x1 input gradients) are those of the committed listing
profiles/resnet_fp16_resource_usage_branch.txt: registers, AGPRs, occupancy and LDS did not move when the tile code got its modes."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def listing():
    from ocpg_amd.csrc import build
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip("hipcc is not installed")
    import kernel_resource_usage
    return kernel_resource_usage.listing(kernel_resource_usage.compile_remarks(["gemm_dgrad_bn.hip"])).splitlines()


def test_new_instantiations_use_no_scratch(listing):
    new = [ln for ln in listing if ln.startswith("gemm_ffn<")]
    names = {ln.split("  ")[0].strip() for ln in new}
    assert names == {"gemm_ffn<%d, %d, %d>" % (tm, tn, mode) for tm, tn in ((128, 128), (64, 128), (64, 64)) for mode in (1, 2)}, names
    for ln in new:
        print(ln)
        assert " scratch    0 " in ln, ln


def test_existing_instantiations_did_not_move(listing):
    committed = [ln.rstrip("\n") for ln in open(os.path.join(ROOT, "profiles", "resnet_fp16_resource_usage_branch.txt"))
                 if ln.startswith("gemm_dgrad_bn")]
    assert len(committed) == 6, committed
    assert [ln for ln in listing if ln.startswith("gemm_dgrad_bn")] == committed
