"""CPU test (-m "not gpu") of the CU resources k_cls_tail (csrc/cls_tail.hip) holds.

The kernel is k_gemm_nt_sk's tile (gemm_sk.hpp) with classifier layer 3 folded in.  It must share a CU the way the launch
it replaces does (DESIGN.md 6 "The register file": two workgroups per CU by registers, four by LDS): no scratch, nothing
spilled, and neither its LDS nor its unified VGPR count above those of the k_gemm_nt_sk<DenseOp, DenseOp> instance of
csrc/dense.hip, the launch classifier 2 was.  Counts of this tree: 172 VGPRs and 33 024 bytes of LDS, both kernels.
(With the Wc3 slice fetched at the kernel's start the count was 180, with the slab's 32-deep dots fully unrolled 208.)"""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def both():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    tail = one(kernel_resources(os.path.join(CSRC, "cls_tail.hip")), "_ZN12_GLOBAL__N_110k_cls_tailE")
    sk = one(kernel_resources(os.path.join(CSRC, "dense.hip")), "_Z12k_gemm_nt_skI8DenseOpTILb0EES1_Lb0EE")
    return tail, sk


def test_cls_tail_holds_no_scratch_and_spills_nothing(both):
    tail, _ = both
    assert tail[".max_flat_workgroup_size"] == 256
    assert tail[".vgpr_spill_count"] == 0 and tail[".private_segment_fixed_size"] == 0


def test_cls_tail_holds_no_more_than_the_split_k_kernel(both):
    tail, sk = both
    print("k_cls_tail", tail, "k_gemm_nt_sk", sk)
    assert tail[".group_segment_fixed_size"] <= sk[".group_segment_fixed_size"]
    assert tail[".vgpr_count"] <= sk[".vgpr_count"]
    # what the two bounds are for: two workgroups of four waves per CU by registers (512 per SIMD), four by LDS (160 KB)
    assert 2 * tail[".vgpr_count"] <= 512 and 4 * tail[".group_segment_fixed_size"] <= 160 * 1024
