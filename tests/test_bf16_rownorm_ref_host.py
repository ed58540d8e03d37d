"""CPU test (-m "not gpu") of tests/bf16_rownorm_ref.py, the reference and envelope that tests/test_gpu_bf16_rownorm_ops.py
holds the bf16 row-norm kernels to: on every case used on the GPU the fp32 emulation of each route sits within a TENTH of
the envelope, and every planted defect — the variance as E[y^2] - mean^2, un-centred weights without a mean sweep, the
unbiased variance, a truncating bf16 store — leaves it on at least one case."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_rownorm_ref as rr


@functools.lru_cache(maxsize=None)
def _case(i):
    inp = rr.inputs(rr.CASES[i])
    return inp, {route: rr.pair_ref(inp, route) for route in ("fused", "materialise")}


@pytest.mark.parametrize("route", ["fused", "materialise"])
@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=[rr.case_id(c) for c in rr.CASES])
def test_emulation_sits_within_a_tenth_of_the_envelope(i, route):
    inp, refs = _case(i)
    want, tol, swant, stol = refs[route]
    pooled, sup = rr.emulate_pair(inp, route)
    r0, bad0 = rr.worst("%s %s pooled" % (rr.case_id(rr.CASES[i]), route), pooled, want, tol)
    r1, bad1 = rr.worst("%s %s super" % (rr.case_id(rr.CASES[i]), route), sup, swant, stol)
    assert bad0 == 0 and bad1 == 0 and r0 <= 0.1 and r1 <= 0.1, (r0, r1)
    empty = torch.from_numpy(inp["lay"].sizes == 0)
    assert float(want[empty].abs().max() if empty.any() else 0.0) == 0.0 and float(tol[empty].abs().max() if empty.any() else 0.0) == 0.0


def test_the_shifted_cases_have_rows_far_from_zero():
    """|row mean| / std >= 30 is what separates a centred variance from E[y^2] - mean^2; the shifted cases have >= 100"""
    seen = 0
    for i, c in enumerate(rr.CASES):
        if not c.shift:
            continue
        inp, _ = _case(i)
        y = inp["feats"].double() @ inp["W"].double().t() + inp["b"].double()
        ratio = float((y.mean(1).abs() / y.std(1, unbiased=False)).min())
        print(rr.case_id(c), "min |row mean| / std", ratio)
        assert ratio >= 100.0
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("name", sorted(rr.DEFECTS))
def test_planted_defect_leaves_the_envelope(name):
    fn, route = rr.DEFECTS[name]
    hits = []
    for i, c in enumerate(rr.CASES):
        inp, refs = _case(i)
        if inp["lay"].N < 2 and name == "unbiased":
            pass
        want, tol, _, _ = refs[route]
        seg = torch.from_numpy(inp["lay"].bbox_idx.copy())
        ratio, bad = rr.worst("%s on %s" % (name, rr.case_id(c)), rr.pool(fn(inp), seg, inp["lay"].P), want, tol)
        if bad:
            hits.append((rr.case_id(c), ratio))
    print(name, hits)
    assert hits, name
    if name == "var_e2":
        # the defect the shifted cases exist for: invisible where the row mean is small, out by far where it is not
        assert all("shift" in h[0] for h in hits) and len(hits) >= 2


@pytest.mark.parametrize("C,M,norm", rr.ROWS_CASES)
def test_row_norm_with_a_bf16_store(C, M, norm):
    inp = rr.rows_inputs(C, M, norm)
    want, tol = rr.rows_ref(inp)
    # half a bf16 spacing is nearly all of this envelope and a round-to-nearest store uses all of it: the emulation is held
    # to the envelope itself here, and to a tenth of the fp32 part before the store
    r, bad = rr.worst("rows C=%d M=%d %s" % (C, M, norm), rr.emulate_rows_h(inp), want, tol)
    assert bad == 0
    z64, delta = rr.rownorm_ref(inp["Y"].double(), None, None, inp["g"], inp["be"], inp["eps"], "rows")
    r32, bad32 = rr.worst("rows fp32 part", rr.emulate_rows(inp["Y"], inp["g"], inp["be"], inp["eps"]), z64, delta)
    assert bad32 == 0 and r32 <= 0.1


def test_a_truncating_store_leaves_the_envelope():
    hits = 0
    for C, M, norm in rr.ROWS_CASES:
        inp = rr.rows_inputs(C, M, norm)
        want, tol = rr.rows_ref(inp)
        hits += rr.worst("truncate C=%d M=%d %s" % (C, M, norm), rr.emulate_rows_h(inp, "truncate"), want, tol)[1] > 0
    assert hits == len(rr.ROWS_CASES)
