"""CPU test (-m "not gpu") of the footprint of the activation-aware instantiations of the bf16 eval fusion kernel
(csrc/fusion_h8.hip k_hfusion_rows8<KD, 1>: act = leakyrelu / prelu, the signed pooling table of segmax.hpp).

The kernel is launched with __launch_bounds__(512, 2): two workgroups share a CU, so an instantiation may hold at most 128
VGPRs, and a spill or a scratch segment would put the walk's registers into memory.  The signed table is the ReLU table
read as unsigned keys, so the LDS must not grow either.  For KD in {64, 128}:

* .max_flat_workgroup_size is 512;
* .vgpr_count <= 128, no spilled register, no scratch;
* .group_segment_fixed_size is no larger than the ReLU instantiation's.

The translation unit is compiled the way tools/kernel_resources.sh does; the numbers are the code object's metadata."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    return kernel_resources(os.path.join(CSRC, "fusion_h8.hip"))


def _inst(kd, act):
    return "_Z15k_hfusion_rows8ILi%dELi%dEE" % (kd, act)


@pytest.mark.parametrize("kd", [64, 128])
def test_act_instantiation_fits_two_workgroups_per_cu(resources, kd):
    act, relu = one(resources, _inst(kd, 1)), one(resources, _inst(kd, 0))
    assert act[".max_flat_workgroup_size"] == 512 == relu[".max_flat_workgroup_size"]
    assert act[".vgpr_count"] <= 128
    assert act[".vgpr_spill_count"] == 0 and act[".private_segment_fixed_size"] == 0
    assert act[".group_segment_fixed_size"] <= relu[".group_segment_fixed_size"]
