"""CPU test (-m "not gpu") of the CU resources the fused row-norm fusion kernel k_fusion_rows_rn (csrc/rownorm.hip) holds.

The kernel is the fusion launch of a --norm layer / instance eval forward: 256 threads = one wave per SIMD own
128 whole rows, keep their split A operand (96 registers at K = 128), two accumulators, the next W tile and the 16 per-row
statistics in registers and walk the column tiles twice.  DESIGN.md states: nothing spilled and no scratch at either K; at
K = 128 256 vector + 32 accumulation registers (288 unified) and 102 KB of LDS, one workgroup per CU; at K = 64 at most
256 unified registers (220 today) and 54 KB of LDS, so that two workgroups share a CU.  The K = 128 bound is 320: an
accumulator handling that shuffles between the two register files (what the "+a" constraint of the kernel's MFMA pin
prevents) needs more than the 32 accumulation registers of the two accumulators.  The translation unit is compiled the way
tools/kernel_resources.sh does and the numbers are read from the code object's metadata (test_kernel_resources_host.py)."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    return kernel_resources(os.path.join(CSRC, "rownorm.hip"))


@pytest.mark.parametrize("kd,vgpr,lds", [(128, 320, 102 * 1024), (64, 256, 54 * 1024)])
def test_fused_kernel_has_no_scratch_and_fits_its_occupancy(resources, kd, vgpr, lds):
    k = one(resources, "_ZN12_GLOBAL__N_116k_fusion_rows_rnILi%dEEE" % kd)
    assert k[".max_flat_workgroup_size"] == 256                         # one wave per SIMD and workgroup
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= vgpr
    assert k[".group_segment_fixed_size"] <= lds
    # LDS is what bounds the workgroups per CU (160 KB): one at K = 128, two at K = 64
    assert 160 * 1024 // k[".group_segment_fixed_size"] == (1 if kd == 128 else 2)


def test_row_kernels_have_no_scratch(resources):
    names = [n for n in resources if "k_rownorm_act" in n or "k_rn_bwd_rows" in n]
    assert len(names) == 4, names                                       # row in registers / re-read, forward / backward
    for n in names:
        k = resources[n]
        print(n[:60], k)
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and k[".vgpr_count"] <= 128
