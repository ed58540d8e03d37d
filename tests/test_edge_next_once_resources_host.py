"""CPU test (-m "not gpu") of the register footprint of k_edge_uv_mlp2_mean<1, true> (csrc/edge.hip), the one-tile edge
kernel that carries the next layer's node side.  It fetches all 48 B fragments of the packed next-layer weight in one batch
after the pass loop; that only pays while four workgroups still share a CU: <= 128 unified VGPRs, nothing spilled, no
scratch.  Compiled and read the way tests/test_kernel_resources_host.py does."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    return kernel_resources(os.path.join(CSRC, "edge.hip"))


def test_one_tile_next_instance_keeps_four_workgroups_per_cu(resources):
    k = one(resources, "_Z19k_edge_uv_mlp2_meanILi1ELb1EE")
    assert k[".vgpr_count"] <= 128
    assert k[".vgpr_spill_count"] == 0
    assert k[".private_segment_fixed_size"] == 0
