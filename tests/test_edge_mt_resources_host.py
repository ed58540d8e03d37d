"""CPU test (-m "not gpu") of the register / scratch / LDS footprint of the several-tiles-per-workgroup edge kernel
(csrc/edge.hip k_edge_mt_uv_mlp2_mean<NEXT>), the shape the eval forward's throughput regime launches.  It exists to hold
fewer CU-microseconds than the one-tile kernel, so it must share a CU exactly like k_edge_uv_mlp2_mean<1, *>: 256 threads
(one wave per SIMD), four workgroups per CU by registers (<= 128 unified VGPRs, allocation rounded up to 8), no spilled
VGPR, no scratch, and four workgroups' LDS inside the CU's 160 KB — for the instance that carries the next layer's node
side and the one that does not.  Compiled and read the way tests/test_kernel_resources_host.py does (hipcc
--offload-arch=gfx950 -O3 --save-temps, the code object metadata in the device assembly)."""
import os

import pytest

from kernel_meta import CSRC, find_hipcc, kernel_resources, one


@pytest.fixture(scope="module")
def resources():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    return kernel_resources(os.path.join(CSRC, "edge.hip"))


@pytest.mark.parametrize("inst", ["ILb1EE", "ILb0EE"])
def test_edge_mt_four_workgroups_per_cu(resources, inst):
    k = one(resources, "_Z22k_edge_mt_uv_mlp2_mean" + inst)
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_count"] <= 128 and 4 * ((k[".vgpr_count"] + 7) // 8 * 8) <= 512
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert 4 * k[".group_segment_fixed_size"] <= 160 * 1024


def test_edge_mt_has_its_own_name(resources):
    # the one-tile instances are found by prefix elsewhere: the new kernel must not match theirs
    assert not [k for k in resources if k.startswith("_Z19k_edge_uv_mlp2_mean") and "mt" in k[:30]]
    assert len([k for k in resources if k.startswith("_Z22k_edge_mt_uv_mlp2_mean")]) == 2
