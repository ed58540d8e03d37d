"""GPU tests (-m gpu) of the stages the bf16-storage eval forward launches for a LEAKY model (act = leakyrelu / prelu),
each element against the float64 model and envelope of tests/bf16_act_ref.py (tests/test_bf16_act_ref_host.py shows on the
CPU that the envelope accepts a literal fp32 evaluation and rejects four wrong kernels, and that these inputs reach the
signed pooling).  The stages run through the entry points internal.hpp exports, which launch what yolat_forward_eval_bf16
launches for such a descriptor:

  yolat_debug_fusion_pair_eval_bf16_act
      route 0  yolat_pool_init_signed + k_hfusion_rows8<64|128, 1> (fusion_h8.hip: key table under an unsigned ds_max, the
               walk from -inf, the signed drain).  Every layout of segmax_layouts.NAMES (a proposal straddling row tiles,
               tiles with more than FX_NP proposals, empty proposals, N = 2 / 31 / 33) at F = 128 with 1 and 2 forced
               column groups (ng = 2: the W double buffer and the drain of the other table; ng = 1); F = 960 in groups of 8
               and 7 tiles; the slopes 0.2, -0.3, 1.4 and 0; a NaN row; the super half at P = 1 and P = 65.  Z starts as
               NaN everywhere: the start values are the call's own.
      route 5  the materialising form (bf16 tile GEMM with fp32 output + yolat_segment_act_max, super block on
               k_hgemm_act) for every other shape: D = 192 and 320, F = 160.  (D = 32 k with k odd is not reachable: the
               forward and the entry take D % 64 == 0 only.)
  yolat_debug_hgemm_eval_bf16_act   k_hgemm_act as prediction_cls.0 / .1 use it: fp32 rows at K = 2304, bf16 rows at
               K = 512, bf16 output, M = 1 / 63 / 64 / 65 (the scalar store of a partial row tile and the staged one)

Every case runs twice and compares bits, and asserts the route and the plan it was written for.  The exercise bars are
asserted on the reference: >= 2 % negative pooled entries for a = 0.2, >= 5 % of the entries of the proposals with two or
more rows different from act(max pre) for a = -0.3 (`many` has one-row proposals only: the share is 0 by identity and is
asserted to be).  The node problem runs with one slope and the super problem with another, so a swap cannot pass.

Largest error / envelope seen on the MI355X (every case prints its own): route 0 pooled 0.711 (`random`, D = 64, a = 0),
its super half 0.272; route 5 pooled 0.072; k_hgemm_act with a bf16 output 0.997 (a bf16 output reaches ~1 by construction:
the envelope is the half spacing of the round-to-nearest store plus the fp32 bound).
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_act_ref as ar
import bf16_eval_ref as er
import segmax_layouts as sl
from bf16_ref import bf, store_envelope

pytestmark = pytest.mark.gpu

P_, I64, CI = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
FUSION = ([P_, I64, I64, I64, P_, P_, P_, I64, I64, I64] + [P_] * 12 + [P_, P_, P_] +
          [CI, ctypes.POINTER(CI), ctypes.POINTER(CI * 2), P_])
HGEMM = [P_, CI, I64, I64, I64, P_, I64, I64, P_, P_, P_, P_, P_, CI, I64, ctypes.POINTER(CI), P_]


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _fn(name, argtypes, restype=CI):
    fn = getattr(_yv()._lib.lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


def _stream():
    return _yv().ops._stream()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(name, got, want, tol):
    ratio, bad = er.worst(name, got, want, tol)
    assert bad == 0, "%s: %d of %d outside the envelope, worst error / envelope %.3f" % (name, bad, got.numel(), ratio)
    return ratio


def _random_layout(N, P, seed):
    g = torch.Generator().manual_seed(seed)
    cut = torch.sort(torch.randint(0, N + 1, (P - 1,), generator=g)).values
    sizes = torch.diff(torch.cat([torch.zeros(1, dtype=torch.long), cut, torch.tensor([N])])).numpy()
    return sl._from_sizes("random_%d_%d" % (N, P), sizes)


def _layout(name):
    return _random_layout(*name) if isinstance(name, tuple) else sl.layout(name)


def _seg_ptr(lay):
    st = torch.from_numpy(sl.starts(lay)).int()
    return torch.cat([st, torch.tensor([lay.N], dtype=torch.int32)]).cuda()


def _fusion_case(name, D, F, a_f, a_s, fold, force, route, plan, nan_row=None):
    """one call of the pair (twice: bit-identical), every element of both halves against float64"""
    lay = _layout(name)
    N, P = lay.N, lay.P
    ZW = 2 * (F + D)
    tag = "act route%d %s D=%d F=%d force=%d a=%g/%g" % (route, lay.name, D, F, force, a_f, a_s)
    inp = {k: v.cuda() for k, v in ar.fusion_act_inputs(lay, D, F).items()}
    if nan_row is not None:
        inp["feats"][nan_row, 3] = float("nan")
    seg64 = er.seg_tensor(lay).cuda()
    seg32, seg_ptr = seg64.int(), _seg_ptr(lay)
    slopes = torch.tensor([a_f, a_s], dtype=torch.float32, device="cuda")
    work_elems = _fn("yolat_fusion_pair_eval_act_work_elems", [I64, I64], ctypes.c_size_t)(N, F)
    work = torch.full((int(work_elems),), float("nan"), device="cuda") if route == 5 else None
    fn = _fn("yolat_debug_fusion_pair_eval_bf16_act", FUSION)

    def run():
        Z = torch.full((P, ZW), float("nan"), device="cuda")      # the pooled start values are the call's own
        Z[:, 2 * F + D:] = inp["S"]
        r, gn = CI(-1), (CI * 2)(-1, -1)
        rc = fn(_ptr(inp["feats"]), D, N, D, _ptr(seg32), _ptr(seg_ptr), _ptr(Z), ZW, P, F, _ptr(inp["W"]), _ptr(inp["Ws"]),
                _ptr(inp["b"]), _ptr(inp["s"]), _ptr(inp["t"]), _ptr(inp["bs"]), _ptr(inp["ss"]), _ptr(inp["ts"]),
                _ptr(inp["Wfold"]) if fold else None, _ptr(inp["tfold"]) if fold else None,
                _ptr(inp["Wfolds"]) if fold else None, _ptr(inp["tfolds"]) if fold else None,
                slopes.data_ptr(), slopes.data_ptr() + 4, _ptr(work), force, ctypes.byref(r), ctypes.byref(gn), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc)
        return Z, r.value, (gn[0], gn[1])

    Z, got_route, got_plan = run()
    Z2, _, _ = run()
    assert got_route == route, (tag, got_route)
    assert got_plan == plan, (tag, got_plan, plan)
    assert torch.equal(_bits(Z), _bits(Z2)), tag + ": two runs differ"
    assert bool(torch.isnan(Z[:, F:F + D]).all()), tag + ": columns F : F + D were written"
    assert torch.equal(Z[:, 2 * F + D:], inp["S"]), tag + ": the super block's input changed"
    af, as_ = ar.slope64(a_f), ar.slope64(a_s)
    if route == 0:
        args = (inp["feats"], inp["Wfold"], "fold", None, None, inp["tfold"], seg64, P)
        swant, stol = ar.super_act_ref(inp["S"], inp["Wfolds"], "fold", None, None, inp["tfolds"], as_)
    else:
        args = (inp["feats"], inp["W"], "tile", inp["b"], inp["s"], inp["t"], seg64, P)
        swant, stol = ar.super_act_ref(inp["S"], inp["Ws"], "tile", inp["bs"], inp["ss"], inp["ts"], as_)
    want, tol, aom = ar.fusion_pool_act_ref(*args, af)
    got = Z[:, :F]
    if nan_row is not None:
        # the NaN row's proposal is NaN in every column (a NaN operand poisons the whole product row); nothing else is
        p = int(seg64[nan_row])
        assert bool(torch.isnan(got[p]).all()), tag + ": the NaN did not reach its proposal"
        keep = torch.ones(P, dtype=torch.bool, device="cuda")
        keep[p] = False
        got, want, tol, aom = got[keep], want[keep], tol[keep], aom[keep]
        assert not bool(torch.isnan(got).any()), tag + ": a NaN outside its proposal"
    else:
        neg, differ, multi = ar.exercise(want, aom, seg64, P)
        print("exercise %s negative %.3f differ %.3f" % (tag, neg, differ))
        if a_f == 0.2:
            assert neg >= 0.02, (tag, neg)
        if a_f == -0.3:
            assert (differ >= 0.05) if multi else (lay.name == "many" and differ == 0.0), (tag, differ)
    ratio = _check(tag + " pooled", got, want, tol)
    sratio = _check(tag + " super", Z[:, F + D:2 * F + D], swant, stol)
    empty = torch.from_numpy(lay.sizes == 0).cuda()
    if bool(empty.any()):
        assert float(Z[empty, :F].abs().max()) == 0.0, tag + ": empty proposals"
    return max(ratio, sratio)


@pytest.mark.parametrize("force", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", sl.NAMES)
def test_h8_act_layouts(name, D, force):
    plan = er.plan_h8(sl.layout(name).N, 128, force)
    assert plan == {1: (1, 2), 2: (2, 1)}[force]
    a_f, a_s = (-0.3, 0.2) if force == 1 else (0.2, -0.3)
    _fusion_case(name, D, 128, a_f, a_s, True, force, 0, plan)


@pytest.mark.parametrize("D", [64, 128])
def test_h8_act_f960_groups_of_8_and_7_tiles(D):
    _fusion_case("straddle", D, 960, -0.3, 1.4, True, 2, 0, (2, 8))


@pytest.mark.parametrize("a", ar.SLOPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ["tiny_then_long", "random"])
def test_h8_act_slopes(name, D, a):
    other = {0.2: 1.4, -0.3: 0.0, 1.4: -0.3, 0.0: 0.2}[a]
    _fusion_case(name, D, 128, a, other, True, 1, 0, (1, 2))


@pytest.mark.parametrize("row", [5, 300, 1099])
def test_h8_act_nan_row_reaches_its_proposal_only(row):
    """row 5: a proposal reduced in the table and stored; row 300: the 600-row proposal shared by three row tiles (merged
    with fx_signed_max); row 1099: the last row"""
    _fusion_case("straddle", 128, 128, -0.3, 0.2, True, 1, 0, (1, 2), nan_row=row)


def test_h8_act_nan_row_beyond_the_table():
    """tiny_then_long: the proposals past position FX_NP of tile 0 go to the pooled matrix directly"""
    lay = sl.layout("tiny_then_long")
    row = int(sl.starts(lay)[50])
    assert 50 >= sl.FX_NP and row < 256
    _fusion_case("tiny_then_long", 64, 128, 0.2, -0.3, True, 2, 0, (2, 1), nan_row=row)


@pytest.mark.parametrize("D", [64, 128])
def test_h8_act_super_half_at_one_and_65_proposals(D):
    _fusion_case("one", D, 128, 0.2, -0.3, True, 1, 0, (1, 2))
    _fusion_case((1000, 65, 4), D, 128, 0.2, -0.3, True, 1, 0, (1, 2))
    _fusion_case((1000, 65, 4), D, 128, -0.3, 1.4, True, 2, 0, (2, 1))


@pytest.mark.parametrize("a", [0.2, -0.3])
@pytest.mark.parametrize("D", [192, 320])
@pytest.mark.parametrize("name", ["straddle", "empty", "small_n2"])
def test_generic_route(name, D, a):
    _fusion_case(name, D, 160, a, 1.4 if a < 0 else -0.3, False, 0, 5, (1, 3))


def test_generic_route_ignores_fold_pointers_it_cannot_use():
    """D = 192 with fold pointers given: still the materialising form"""
    _fusion_case("straddle", 192, 160, -0.3, 0.2, True, 0, 5, (1, 3))


# ---------------------------------------------------------------------------------------------
# the classifier's GEMM with the activation in its epilogue
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [-0.3, 1.4])
@pytest.mark.parametrize("K,Nout", [(2304, 512), (512, 256)])
@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_hgemm_act_bf16_out(M, K, Nout, a):
    a_f32 = K == 2304                                        # prediction_cls.0 reads the fp32 Z, .1 the bf16 c1
    tg = torch.Generator().manual_seed(M + 3 * K + Nout)
    A = torch.randn(M, K, generator=tg)
    A = (A if a_f32 else A.to(torch.bfloat16)).cuda()
    W = (torch.randn(Nout, K, generator=tg) / K ** 0.5).to(torch.bfloat16).cuda()
    b, s, t = (v.cuda() for v in er.bn_vectors(Nout, tg))
    slope = torch.tensor([a], dtype=torch.float32, device="cuda")
    fn = _fn("yolat_debug_hgemm_eval_bf16_act", HGEMM)

    def run():
        Y = torch.full((M, Nout), float("nan"), dtype=torch.bfloat16, device="cuda")
        tf = CI(-1)
        rc = fn(_ptr(A), int(a_f32), K, M, K, _ptr(W), K, Nout, _ptr(b), _ptr(s), _ptr(t), _ptr(slope), _ptr(Y), 1, Nout,
                ctypes.byref(tf), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return Y, tf.value

    Y, form = run()
    assert form == 0
    assert torch.equal(_bits(Y), _bits(run()[0])), "two runs differ"
    want, env, val = ar.stage_act_ref(bf(A) if a_f32 else er.widen(A), er.widen(W), "tile", b, s, t, ar.slope64(a))
    assert float((val < 0).double().mean()) > 0.2            # the activation's other branch is taken
    _check("hgemm_act M=%d K=%d Nout=%d a=%g" % (M, K, Nout, a), Y, want, store_envelope(want, env))


def test_hgemm_act_slope_is_read_by_every_launch():
    """an in-place edit of the slope is seen by the next launch"""
    tg = torch.Generator().manual_seed(9)
    A = torch.randn(64, 512, generator=tg).to(torch.bfloat16).cuda()
    W = (torch.randn(256, 512, generator=tg) / 512 ** 0.5).to(torch.bfloat16).cuda()
    slope = torch.tensor([0.2], dtype=torch.float32, device="cuda")
    fn = _fn("yolat_debug_hgemm_eval_bf16_act", HGEMM)
    outs = []
    for a in (0.2, -0.3):
        slope.fill_(a)
        Y = torch.empty(64, 256, dtype=torch.bfloat16, device="cuda")
        assert fn(_ptr(A), 0, 512, 64, 512, _ptr(W), 512, 256, None, None, None, _ptr(slope), _ptr(Y), 1, 256, None,
                  _stream()) == 0
        torch.cuda.synchronize()
        want, env, _ = ar.stage_act_ref(er.widen(A), er.widen(W), "tile", None, None, None, ar.slope64(a))
        _check("hgemm_act slope edit a=%g" % a, Y, want, store_envelope(want, env))
        outs.append(Y)
    assert not torch.equal(_bits(outs[0]), _bits(outs[1]))
