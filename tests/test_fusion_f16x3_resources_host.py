"""CPU test (-m "not gpu") of the footprint of the f16x3 eval fusion kernel (csrc/fusion_f16x3.hip k_fusion_rows_f16x3).

Half the matrix work is one half of the claim; the other is what the launch holds on a CU while it runs (DESIGN.md 6 "The
loaded regime": the fusion launch is the largest reservation of a forward).  Against k_fusion_rows_x6<128, true>, the
instance the cfg-2 forward launches (234 unified VGPRs, 104448 bytes of LDS):

* the K = 128 instance with the rider holds 208 unified VGPRs — A's fragments are 64 registers instead of 96 — and 69632
  bytes of LDS: two W tiles of 2 x 64 x (128 + 8) halves, exactly the size of the prologue's eight transposition tiles;
* no spilled register, no scratch;
* both counts are below the x6 instance's, for every (rider, activation) instance.

The translation unit is compiled the way tools/kernel_resources.sh does; the numbers are the code objects' metadata."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    # (the x6 siblings are fusion_x6.hip's)
    return {**kernel_resources(os.path.join(CSRC, "fusion_f16x3.hip")), **kernel_resources(os.path.join(CSRC, "fusion_x6.hip"))}


def _inst(kernel, kd, rider, act):
    return "_Z%d%sILi%dELb%dELi%dEE" % (len(kernel), kernel, kd, rider, act)


def test_f16x3_k128_rider_instance_holds_what_the_build_gives(resources):
    k = one(resources, _inst("k_fusion_rows_f16x3", 128, 1, 0))
    assert k[".max_flat_workgroup_size"] == 512
    assert k[".vgpr_count"] == 208
    assert k[".group_segment_fixed_size"] == 69632 == 2 * 2 * 64 * (128 + 8) * 2
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rider", [0, 1])
@pytest.mark.parametrize("kd", [64, 128])
def test_f16x3_instances_are_leaner_than_their_x6_siblings(resources, kd, rider, act):
    new = one(resources, _inst("k_fusion_rows_f16x3", kd, rider, act))
    old = one(resources, _inst("k_fusion_rows_x6", kd, rider, act))
    assert new[".vgpr_spill_count"] == 0 and new[".private_segment_fixed_size"] == 0
    assert new[".vgpr_count"] < old[".vgpr_count"]
    assert new[".group_segment_fixed_size"] < old[".group_segment_fixed_size"]
    assert new[".max_flat_workgroup_size"] == old[".max_flat_workgroup_size"]
