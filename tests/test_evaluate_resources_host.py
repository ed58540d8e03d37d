"""CPU test (-m "not gpu") of the code objects of csrc/evaluate.hip: the rows kernel of the asynchronous evaluation is a
latency-bound launch of a few hundred to a few thousand rows with a 32-float row in registers — a spill would be a scratch
round trip per class — and the final kernel is one workgroup.  Neither may spill or use a private segment."""
import os

import pytest

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

from kernel_meta import CSRC, find_hipcc, kernel_resources


def test_rows_and_final_kernels_do_not_spill():
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    res = kernel_resources(os.path.join(CSRC, "evaluate.hip"))
    rows = {k: v for k, v in res.items() if "k_eval_rows" in k}
    final = {k: v for k, v in res.items() if "k_eval_final" in k}
    assert len(rows) == 2 and len(final) == 2, sorted(res)          # softmax / BCE instances of each
    for name, k in list(rows.items()) + list(final.items()):
        print(name[:48], k)
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
    for name, k in rows.items():
        assert k[".max_flat_workgroup_size"] == 256
        assert k[".vgpr_count"] <= 64                                # the loss kernels' budget: 8 waves per SIMD
        # the LDS confusion table (K <= 32: 4 KB) + the hit counter + the 256-float tree
        assert k[".group_segment_fixed_size"] == 32 * 32 * 4 + 4 + 256 * 4
    for name, k in final.items():
        assert k[".max_flat_workgroup_size"] == 1024 and k[".group_segment_fixed_size"] == 1024 * 4
