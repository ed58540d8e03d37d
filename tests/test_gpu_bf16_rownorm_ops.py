"""GPU tests (-m gpu) of the bf16-storage eval forward's stages behind a row norm (--norm layer / instance), each element
against the float64 reference and envelope of tests/bf16_rownorm_ref.py (tests/test_bf16_rownorm_ref_host.py shows on the
CPU that the envelope holds an fp32 emulation of each route within a tenth of itself and rejects five wrong kernels).  The
stages run through the entry points internal.hpp exports for tools and tests, which launch what yolat_forward_eval_bf16
launches for such a model:

  yolat_debug_fusion_pair_eval_bf16_rn   fusion block + row norm + ReLU + per-proposal max | fusion_block_super.  Every case
      of bf16_rownorm_ref.CASES on both routes, the reported route asserted:
        route 6  k_hfusion_rows8_rn<64 | 128> (fusion_h8_rn.hip) on the centred fold weights, one launch
        route 7  the materialising form (bf16 tile GEMM -> yolat_rownorm_act -> k_rn_range_max) on the plain weights; D = 192
                 lands here whatever rn_route says
      The cases: D = 64 / 128, F = 64 (one column tile) / 1024, layer / instance (gamma NULL), N = 1, N = 257 (the last row
      alone in its workgroup), one proposal over four row tiles, one-node proposals, 62 and 256 proposals in a row tile (more
      than the FX_NP = 32 of the LDS table), empty proposals (exactly 0), a zero row with zero bias (exactly relu(beta)), rows
      with |row mean| / std > 300.  Columns F : F + D of Z stay NaN, two runs are bit-identical, and a declined call (misaligned
      rows, D = 96) leaves a NaN-filled Z untouched.
  yolat_debug_rownorm_act_bf16           k_rownorm_act_h at C = 256 / 512, M = 1 / 63 / 65, both norms, against the float64
      norm and the envelope of ONE bf16 rounding.

The float64 references are computed on the device, once per case."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_rownorm_ref as rr

pytestmark = pytest.mark.gpu

P_, I64, CI, CF = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
FUSED, MATERIALISE = 1, 2              # YOLAT_RN_ROUTE_*
UNSUPPORTED = -2


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _fn(name, argtypes):
    fn = getattr(_yv()._lib.lib, name)
    fn.restype = CI
    fn.argtypes = argtypes
    return fn


def _pair_fn():
    return _fn("yolat_debug_fusion_pair_eval_bf16_rn", [P_, I64, I64, I64, P_, P_, I64, I64, I64] + [P_] * 12 +
               [CF, CI, P_, ctypes.POINTER(CI), ctypes.POINTER(CI * 2), P_])


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(i):
    """operands on the device and the float64 references of both routes, computed once"""
    c = rr.CASES[i]
    inp = rr.inputs(c)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    dev["seg32"] = torch.from_numpy(inp["lay"].bbox_idx.copy()).int().cuda()
    refs = {route: rr.pair_ref(inp, route, "cuda") for route in ("fused", "materialise")}
    return c, inp, dev, refs


def _run(c, inp, dev, rn_route, feats=None, D=None):
    """one call on a fresh Z; returns (rc, Z, reported route)"""
    lay, F = inp["lay"], c.F
    D = c.D if D is None else D
    N, P, ZW = lay.N, lay.P, 2 * (F + D)
    Z = torch.zeros(P, ZW, device="cuda")
    Z[:, F:F + D] = float("nan")                      # the pooling prologue's maxima: not this launch's
    Z[:, F + D:2 * F + D] = float("nan")              # the super output: written in full
    Z[:, 2 * F + D:2 * F + D + c.D] = dev["S"]
    work = torch.empty(int(_yv()._lib.lib.yolat_fusion_pair_eval_rn_work_elems(N, F)), device="cuda")
    r, gn = CI(-1), (CI * 2)(-1, -1)
    feats = dev["feats"] if feats is None else feats
    rc = _pair_fn()(feats.data_ptr(), D, N, D, dev["seg32"].data_ptr(), Z.data_ptr(), ZW, P, F, dev["W"].data_ptr(),
                    dev["Ws"].data_ptr(), dev["b"].data_ptr(), dev["bs"].data_ptr(), dev["Wc"].data_ptr(),
                    dev["bc"].data_ptr(), dev["Wcs"].data_ptr(), dev["bcs"].data_ptr(), _ptr(dev["g"]), _ptr(dev["be"]),
                    _ptr(dev["gs"]), _ptr(dev["bes"]), inp["eps"], rn_route, work.data_ptr(), ctypes.byref(r), ctypes.byref(gn),
                    _yv().ops._stream())
    torch.cuda.synchronize()
    return rc, Z, r.value


PAIR = [(i, route) for i, c in enumerate(rr.CASES) for route in ("fused", "materialise") if route == "materialise" or c.D in (64, 128)]


@pytest.mark.parametrize("i,route", PAIR, ids=["%s-%s" % (rr.case_id(rr.CASES[i]), r) for i, r in PAIR])
def test_fusion_pair_vs_fp64(i, route):
    c, inp, dev, refs = _case(i)
    F, D, lay = c.F, c.D, inp["lay"]
    rc, Z, reported = _run(c, inp, dev, FUSED if route == "fused" else MATERIALISE)
    assert rc == 0 and reported == (6 if route == "fused" else 7)
    rc2, Z2, _ = _run(c, inp, dev, FUSED if route == "fused" else MATERIALISE)
    assert rc2 == 0 and torch.equal(_bits(Z[:, :F]), _bits(Z2[:, :F])) and torch.equal(_bits(Z[:, F + D:2 * F + D]), _bits(Z2[:, F + D:2 * F + D]))
    want, tol, swant, stol = refs[route]
    tag = "%s %s" % (rr.case_id(c), route)
    r0, bad0 = rr.worst(tag + " pooled", Z[:, :F], want, tol)
    r1, bad1 = rr.worst(tag + " super", Z[:, F + D:2 * F + D], swant, stol)
    assert bad0 == 0, "%s: %d pooled elements outside the envelope, worst %.3f" % (tag, bad0, r0)
    assert bad1 == 0, "%s: %d super elements outside the envelope, worst %.3f" % (tag, bad1, r1)
    assert bool(torch.isnan(Z[:, F:F + D]).all())                         # not this launch's columns
    assert torch.equal(Z[:, 2 * F + D:], Z2[:, 2 * F + D:])              # the super input is read only
    empty = torch.from_numpy(lay.sizes == 0).cuda()
    if bool(empty.any()):
        assert float(Z[empty][:, :F].abs().max()) == 0.0                  # exactly 0, not within a tolerance
    if c.zero_row:
        # a zero row with zero bias has zero deviations: exactly relu(beta), 0 for the instance norm; it is the last proposal
        for got, be in ((Z[-1, :F], dev["be"]), (Z[-1, F + D:2 * F + D], dev["bes"])):
            exact = torch.relu(be) if be is not None else torch.zeros(F, device="cuda")
            assert torch.equal(_bits(got), _bits(exact))


def test_d192_takes_the_materialising_route_whatever_the_descriptor_says():
    i = [k for k, c in enumerate(rr.CASES) if c.D == 192][0]
    c, inp, dev, refs = _case(i)
    rc, Z, reported = _run(c, inp, dev, FUSED)
    assert rc == 0 and reported == 7
    want, tol, _, _ = refs["materialise"]
    assert rr.worst("D=192 asked for fused", Z[:, :c.F], want, tol)[1] == 0


@pytest.mark.parametrize("rn_route", [FUSED, MATERIALISE])
def test_declined_calls_write_nothing(rn_route):
    c, inp, dev, _ = _case(0)
    lay, F, D = inp["lay"], c.F, c.D
    fn = _pair_fn()
    Z = torch.full((lay.P, 2 * (F + D)), float("nan"), device="cuda")
    work = torch.full((int(_yv()._lib.lib.yolat_fusion_pair_eval_rn_work_elems(lay.N, F)),), float("nan"), device="cuda")
    shifted = torch.zeros(lay.N * D + 8, dtype=torch.bfloat16, device="cuda")[4:]          # rows 8 bytes off a 16-byte boundary

    def call(feats, d):
        return fn(feats.data_ptr(), d, lay.N, d, dev["seg32"].data_ptr(), Z.data_ptr(), 2 * (F + D), lay.P, F, dev["W"].data_ptr(),
                  dev["Ws"].data_ptr(), dev["b"].data_ptr(), dev["bs"].data_ptr(), dev["Wc"].data_ptr(), dev["bc"].data_ptr(),
                  dev["Wcs"].data_ptr(), dev["bcs"].data_ptr(), _ptr(dev["g"]), _ptr(dev["be"]), _ptr(dev["gs"]), _ptr(dev["bes"]),
                  inp["eps"], rn_route, work.data_ptr(), None, None, _yv().ops._stream())

    assert shifted.data_ptr() % 16 == 8
    assert call(shifted, D) == UNSUPPORTED
    assert call(dev["feats"], 96) == UNSUPPORTED                          # D = 96 (the buffers are larger than 96 columns need)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Z).all()) and bool(torch.isnan(work).all())


@pytest.mark.parametrize("C,M,norm", rr.ROWS_CASES)
def test_rownorm_act_bf16_vs_fp64(C, M, norm):
    inp = rr.rows_inputs(C, M, norm)
    fn = _fn("yolat_debug_rownorm_act_bf16", [P_, I64, I64, I64, P_, P_, CF, P_, I64, P_])
    Y = inp["Y"].cuda()
    g, be = (inp["g"].cuda(), inp["be"].cuda()) if inp["g"] is not None else (None, None)
    outs = []
    for _ in range(2):
        Z = torch.full((M + 1, C), float("nan"), dtype=torch.bfloat16, device="cuda")     # a guard row behind the last one
        assert fn(Y.data_ptr(), C, M, C, _ptr(g), _ptr(be), inp["eps"], Z.data_ptr(), C, _yv().ops._stream()) == 0
        torch.cuda.synchronize()
        outs.append(Z)
    assert torch.equal(outs[0][:M].view(torch.int16), outs[1][:M].view(torch.int16))
    assert bool(torch.isnan(outs[0][M]).all())
    want, tol = rr.rows_ref(inp, "cuda")
    r, bad = rr.worst("rownorm_h C=%d M=%d %s" % (C, M, norm), outs[0][:M], want, tol)
    assert bad == 0, (r, bad)
    assert float(outs[0][:M].float().min()) >= 0.0
    # in place is declined: the bf16 rows would overlap fp32 rows that other waves still read
    assert fn(Y.data_ptr(), C, M, C, _ptr(g), _ptr(be), inp["eps"], Y.data_ptr(), C, _yv().ops._stream()) == -1
