"""CPU test (-m "not gpu") of the CU resources k_gemm_nt_sk_x6dma (csrc/linear_sk_x6.hip) holds.

The kernel is classifier 1 of the loaded eval forward (DESIGN.md 6 "The loaded regime"): 208 workgroups of 512 threads =
two waves per SIMD, and two workgroups are meant to share a CU, as with the fp32-input kernel it replaces.  That takes
<= 128 unified VGPRs per lane (4 waves per SIMD x 128 = the 512 of a SIMD) with nothing spilled and no scratch, and an LDS
footprint of at most half a CU's 160 KB.  The translation unit is compiled the way tools/kernel_resources.sh does and
the numbers are read from the code object's metadata in the device assembly (test_kernel_resources_host.py)."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    return kernel_resources(os.path.join(CSRC, "linear_sk_x6.hip"))


def test_sk_x6dma_fits_two_workgroups_per_cu(resources):
    k = one(resources, "_Z18k_gemm_nt_sk_x6dma")
    assert k[".max_flat_workgroup_size"] == 512                        # 2 waves per SIMD
    assert k[".vgpr_count"] <= 128
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".group_segment_fixed_size"] <= 80 * 1024
