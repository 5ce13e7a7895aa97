"""The ring form of the 3x3 weight gradient (csrc/conv3x3_wgrad_ring_kernel.h), the part that needs no GPU: the compiler's own resource
remarks for csrc/conv3x3_wgrad.hip (tools/kernel_resource_usage.py).  The ring instantiations use no scratch and reach two waves per SIMD
(a workgroup is eight waves: one workgroup per CU is two per SIMD), and the lines of the present kernel's instantiations are those of the
listing taken at the parent commit, profiles/wgrad_ring_resource_usage_parent.txt: the second kernel family beside it moved nothing."""
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
    return kernel_resource_usage.listing(kernel_resource_usage.compile_remarks(["conv3x3_wgrad.hip"])).splitlines()


def test_ring_instantiations_use_no_scratch_at_two_waves_per_simd(listing):
    new = [ln for ln in listing if ln.startswith("conv3x3_wgrad_ring")]
    names = {ln.split("  ")[0].strip() for ln in new}
    # <stride, segment, k steps of 16 pixels per output row>: a 64-pixel segment takes up to four, a 32-pixel one up to two
    args = ["1, 64, %d" % ks for ks in (1, 2, 3, 4)] + ["2, 32, %d" % ks for ks in (1, 2)]
    assert names == {"%s<%s>" % (k, a) for k in ("conv3x3_wgrad_ring", "conv3x3_wgrad_ring_f16") for a in args}, names
    for ln in new:
        print(ln)
        assert " scratch    0 " in ln, ln
        assert int(ln.split("occupancy")[1].split()[0]) >= 2, ln


def test_present_instantiations_did_not_move(listing):
    committed = [ln.rstrip("\n") for ln in open(os.path.join(ROOT, "profiles", "wgrad_ring_resource_usage_parent.txt"))]
    assert len(committed) == 4 and all(ln.startswith("conv3x3_wgrad<") or ln.startswith("conv3x3_wgrad_f16<") for ln in committed), committed
    assert [ln for ln in listing if not ln.startswith("conv3x3_wgrad_ring")] == committed
