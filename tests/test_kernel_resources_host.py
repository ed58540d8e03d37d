"""CPU test (-m "not gpu") of the register / scratch footprint of the small-graph edge and preparation kernels.

Under load (32 forwards in flight, DESIGN.md 6 "The loaded regime") throughput follows the CU resources a launch holds, and
for these kernels the register file — 512 unified VGPRs (arch + accumulation) per lane per SIMD, a wave's allocation
rounded up to 8 — is the tight one, before LDS and wave slots.  The bounds held here are what the residency the sources
claim needs, not what the compiler happens to give:

* k_edge_uv_mlp2_mean<1, *> (256 threads = 1 wave per SIMD): four workgroups per CU = 4 waves per SIMD -> <= 128, and
  no spilled VGPR / no scratch, for the instance with the next layer's node side and the one without;
* k_edge_uv_mlp2_mean<4, false> (the ~1-edge-per-node shape) keeps its open bound: not above the 180 it had before the
  NG == 1 instances were bound, and no scratch;
* k_prep_small (1024 threads = 4 waves per SIMD) is the form it was: one workgroup per CU by registers, which is
  what its source now says; whatever form it takes, its allocation must fit a SIMD (4 x alloc <= 512) and it must not
  spill or use scratch.

The two translation units are compiled the way tools/kernel_resources.sh does (hipcc --offload-arch=gfx950 -O3
--save-temps) and the numbers are read from the code objects' metadata in the device assembly."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    res = {}
    for name in ("edge.hip", "graph.hip"):
        res.update(kernel_resources(os.path.join(CSRC, name)))
    return res


def alloc(vgprs):
    return (vgprs + 7) // 8 * 8


@pytest.mark.parametrize("inst", ["ILi1ELb1EE", "ILi1ELb0EE"])
def test_edge_tiles_ng1_four_workgroups_per_cu(resources, inst):
    k = one(resources, "_Z19k_edge_uv_mlp2_mean" + inst)
    assert k[".max_flat_workgroup_size"] == 256                       # 1 wave per SIMD
    assert k[".vgpr_count"] <= 128 and 4 * alloc(k[".vgpr_count"]) <= 512
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert 4 * k[".group_segment_fixed_size"] <= 160 * 1024


def test_edge_tiles_ng1_without_next_carries_no_fragments(resources):
    # the instance without the next layer's node side is the leaner one: it holds no B fragments at all
    a = one(resources, "_Z19k_edge_uv_mlp2_meanILi1ELb0EE")
    b = one(resources, "_Z19k_edge_uv_mlp2_meanILi1ELb1EE")
    assert a[".vgpr_count"] <= b[".vgpr_count"]


def test_edge_tiles_ng4_did_not_grow(resources):
    k = one(resources, "_Z19k_edge_uv_mlp2_meanILi4E")
    assert k[".vgpr_count"] <= 180
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0


def test_prep_small_fits_without_scratch(resources):
    k = one(resources, "_Z12k_prep_small")
    waves_per_simd = k[".max_flat_workgroup_size"] // 256
    assert waves_per_simd * alloc(k[".vgpr_count"]) <= 512
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".group_segment_fixed_size"] <= 160 * 1024
