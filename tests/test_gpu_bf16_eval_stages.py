"""GPU tests (-m gpu) of the dense stages of the bf16-storage eval forward, each element against the float64 model and
envelope of tests/bf16_eval_ref.py (tests/test_bf16_eval_ref_host.py shows on the CPU that the envelope accepts an fp32
emulation of every stage and rejects eight wrong kernels).  The stages run through the entry points internal.hpp exports
for tools and tests, which launch what yolat_forward_eval_bf16 launches, routed by the forward's own function:

  yolat_debug_fusion_pair_eval_bf16   fusion block + per-proposal max | fusion_block_super, one launch.  Every case asserts
      the reported route and the (groups, ng) of the node problem, so a case cannot stop reaching what it was written for:
        route 0  k_hfusion_rows8<64|128> (fusion_h8.hip), folded weights: every layout planned (ng = 1 at these N);
                 `straddle`, `tiny_then_long`, `one`, `random` with 1, 3 and 8 forced groups (ng = 16, 6 with a short last
                 group of 4 tiles, 2: the W double buffer, the drain of the other table, the t0 / t1 refetch); F = 960 in
                 groups of 8 and 7 tiles; N = 66 000 where `split` itself picks groups = 1, ng = 16
        route 1  k_hfusion_rows<1,128>, fold pointers NULL, F = 160 (half-masked last column tile), ng = 3 and ng = 1
        route 2  k_hfusion_rows<1,256>, D = 192 (the zero fill of the LDS image) and 256, F = 160 and 1024, ng = 1, 3,
                 16, and N = 8 229 where the plan itself gives ng = 2
        route 3  k_hgemm_two<1>, D = 320;   route 4  k_hgemm_two<2>, D = 320, N = 65 665
      The super half is checked at the layout's P (1 .. 65 835); columns F : F + D of Z stay NaN; two runs are bit-identical.
  yolat_debug_pool_prepare_bf16       k_pool_prepare_h: maxima and the zero block bit-equal, the mean within its bound;
      `many` covers the 65535-proposal chunk
  yolat_debug_node_uv_eval_bf16       k_hgemm_node3: UV (bf16), root (fp32), s_out (bf16), inputs and s_out dense and as a
      64-column slot of a 128-wide buffer
  yolat_debug_hgemm_eval_bf16         launch_hgemm as the classifier uses it: fp32 rows rounded while staging, K = 2304
      through the two-deep prefetch ring, K / 64 odd, bf16 output with folded BatchNorm + ReLU, fp32 logits on a masked
      tile (Nout = 17, 1), and the 64 x 128 tile form k_hgemm<1,2>

Inputs: non-negative bf16 activations drawn as bf16, tie proposals, s = +0 / -0.0 columns with t > 0, a quarter of the
scales negative, closed columns (t = -50).  The float64 references are computed on the device.

Largest error / envelope seen on the MI355X, per route (every case prints its own):
  fusion pair, pooled max   route 0 0.843 (N = 66 000; `many` 0.812)   route 1 0.146   route 2 0.130   route 3 0.072
                            route 4 0.009;   super half 0.015 / 0.015 / 0.004 / 0.003 / 0.003
  pooling prologue, mean    0.159 (maxima and zero block bit-equal)
  node side                 UV 1.000   root 0.012   s_out 0.998
  classifier GEMM           fp32 rows -> bf16 0.999   bf16 rows -> bf16 0.996   fp32 logits 0.003   <1,2> form 1.000
Route 0 sits highest: its shift is the accumulators' initial value, so it is rounded in every MFMA step, where the
envelope prices it as one epilogue term; the elements nearest the envelope belong to a column with |s| = 1.5e-3 under a
shift of 0.336 and are off by 6.9 2^-24 |t| (D = 128: 8 MFMA steps).
A bf16 output reaches 1.000 by construction: its envelope is the half spacing of the round-to-nearest store plus delta,
and a value next to a rounding midpoint uses all of the half spacing.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_eval_ref as er
import segmax_layouts as sl
from bf16_ref import bf, store_envelope

pytestmark = pytest.mark.gpu

P_, I64, CI = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _fn(name, argtypes):
    fn = getattr(_yv()._lib.lib, name)
    fn.restype = CI
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


# ---------------------------------------------------------------------------------------------
# fusion pair
# ---------------------------------------------------------------------------------------------
def _random_layout(N, P, seed):
    g = torch.Generator().manual_seed(seed)
    cut = torch.sort(torch.randint(0, N + 1, (P - 1,), generator=g)).values
    sizes = torch.diff(torch.cat([torch.zeros(1, dtype=torch.long), cut, torch.tensor([N])])).numpy()
    return sl._from_sizes("random_%d_%d" % (N, P), sizes)


def _layout(name):
    if isinstance(name, tuple):
        return _random_layout(*name)
    return sl.layout(name)


def _fusion_case(name, D, F, fold, force, route, plan):
    """one launch of the pair (twice: bit-identical), every element of both halves against float64"""
    lay = _layout(name)
    N, P = lay.N, lay.P
    ZW = 2 * (F + D)
    tag = "route%d %s D=%d F=%d force=%d" % (route, lay.name, D, F, force)
    inp = {k: v.cuda() for k, v in er.fusion_inputs(lay, D, F, 31 * N + 7 * D + F).items()}
    seg64 = er.seg_tensor(lay).cuda()
    seg32 = seg64.int()
    fn = _fn("yolat_debug_fusion_pair_eval_bf16",
             [P_, I64, I64, I64, P_, P_, I64, I64, I64] + [P_] * 12 + [CI, ctypes.POINTER(CI), ctypes.POINTER(CI * 2), P_])

    def run():
        Z = torch.zeros(P, ZW, device="cuda")
        Z[:, F:F + D] = float("nan")                      # the pooling prologue's maxima: not this launch's
        Z[:, F + D:2 * F + D] = float("nan")              # the super output: written in full
        Z[:, 2 * F + D:] = inp["S"]
        r, gn = CI(-1), (CI * 2)(-1, -1)
        rc = fn(_ptr(inp["feats"]), D, N, D, _ptr(seg32), _ptr(Z), ZW, P, F, _ptr(inp["W"]), _ptr(inp["Ws"]),
                _ptr(inp["b"]), _ptr(inp["s"]), _ptr(inp["t"]), _ptr(inp["bs"]), _ptr(inp["ss"]), _ptr(inp["ts"]),
                _ptr(inp["Wfold"]) if fold else None, _ptr(inp["tfold"]) if fold else None,
                _ptr(inp["Wfolds"]) if fold else None, _ptr(inp["tfolds"]) if fold else None, force, ctypes.byref(r),
                ctypes.byref(gn), _stream())
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
    form = "fold" if route == 0 else ("rows" if route in (1, 2) else "tile")
    sform = "fold" if route == 0 else "tile"
    if form == "fold":
        want, tol = er.fusion_pool_ref(inp["feats"], inp["Wfold"], form, None, None, inp["tfold"], seg64, P)
        swant, stol = er.super_ref(inp["S"], inp["Wfolds"], sform, None, None, inp["tfolds"])
    else:
        want, tol = er.fusion_pool_ref(inp["feats"], inp["W"], form, inp["b"], inp["s"], inp["t"], seg64, P)
        swant, stol = er.super_ref(inp["S"], inp["Ws"], sform, inp["bs"], inp["ss"], inp["ts"])
    ratio = _check(tag + " pooled", Z[:, :F], want, tol)
    sratio = _check(tag + " super", Z[:, F + D:2 * F + D], swant, stol)
    assert float(Z[:, 2:F:16].abs().max()) == 0.0, tag + ": closed columns"
    empty = torch.from_numpy(lay.sizes == 0).cuda()
    if bool(empty.any()):
        assert float(Z[empty, :F].abs().max()) == 0.0, tag + ": empty proposals"
    return max(ratio, sratio)


H8_FORCED = [(name, g) for name in ("straddle", "tiny_then_long", "one", "random") for g in (1, 3, 8)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", sl.NAMES)
def test_fusion_h8_planned(name, D):
    F = 64 if name == "many" else 1024
    plan = er.plan_h8(sl.layout(name).N, F)
    assert plan[1] == 1                                   # what the forward's sizes in tests reach: one tile per workgroup
    _fusion_case(name, D, F, True, 0, 0, plan)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name,groups", H8_FORCED, ids=["%s-g%d" % c for c in H8_FORCED])
def test_fusion_h8_forced_groups(name, groups, D):
    plan = {1: (1, 16), 3: (3, 6), 8: (8, 2)}[groups]
    _fusion_case(name, D, 1024, True, groups, 0, plan)


@pytest.mark.parametrize("D", [64, 128])
def test_fusion_h8_f960_groups_of_8_and_7_tiles(D):
    _fusion_case("straddle", D, 960, True, 2, 0, (2, 8))


def test_fusion_h8_split_picks_one_group_at_66000_rows():
    _fusion_case((66000, 2000, 1), 128, 1024, True, 0, 0, (1, 16))


@pytest.mark.parametrize("force", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ["straddle", "tiny_then_long", "empty"])
def test_fusion_rows128_unfolded(name, D, force):
    _fusion_case(name, D, 160, False, force, 1, {1: (1, 3), 4: (3, 1)}[force])


@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("F", [160, 1024])
@pytest.mark.parametrize("D", [192, 256])
@pytest.mark.parametrize("name", ["straddle", "tiny_then_long", "empty"])
def test_fusion_rows256(name, D, F, force):
    plan = er.plan_rows(sl.layout(name).N, F, force)
    assert plan == {(160, 0): (3, 1), (160, 1): (1, 3), (1024, 0): (16, 1), (1024, 1): (1, 16)}[(F, force)]
    _fusion_case(name, D, F, D == 256, force, 2, plan)    # (D = 256: the fold pointers do not change the route)


@pytest.mark.parametrize("D", [192, 256])
def test_fusion_rows256_planned_split_walks_two_tiles(D):
    plan = er.plan_rows(8192 + 37, 1024)
    assert plan == (8, 2)
    _fusion_case((8192 + 37, 300, 2), D, 1024, False, 0, 2, plan)


@pytest.mark.parametrize("F", [160, 1024])
@pytest.mark.parametrize("name", ["straddle", "empty", "small_n2"])
def test_fusion_hgemm_two_64(name, F):
    _fusion_case(name, 320, F, False, 0, 3, (-(-F // 64), 1))


def test_fusion_hgemm_two_128():
    _fusion_case((65536 + 129, 1500, 3), 320, 512, False, 0, 4, (4, 1))


def test_fusion_super_half_at_one_and_65835_proposals():
    """P = 1 (`one`) and P = 65 835 (`many`) are cases of test_fusion_h8_planned; the unfolded super block (hgemm_tile
    with fp32 rows) at the same two P"""
    _fusion_case("one", 64, 160, False, 0, 1, er.plan_rows(sl.layout("one").N, 160))
    _fusion_case("many", 64, 64, False, 0, 1, (1, 1))


# ---------------------------------------------------------------------------------------------
# pooling prologue
# ---------------------------------------------------------------------------------------------
POOL_SHAPES = [(64, 64), (64, 1024), (128, 64), (128, 1024), (320, 64), (320, 1024)]


@pytest.mark.parametrize("name", sl.NAMES)
def test_pool_prepare_vs_fp64(name):
    lay = sl.layout(name)
    N, P = lay.N, lay.P
    seg = er.seg_tensor(lay).cuda()
    seg_ptr = torch.from_numpy(sl.starts(lay)).int()
    seg_ptr = torch.cat([seg_ptr, torch.tensor([N], dtype=torch.int32)]).cuda()
    fn = _fn("yolat_debug_pool_prepare_bf16", [P_, P_, I64, I64, I64, P_, I64, P_, I64, P_])
    worst = 0.0
    for D, F in ([(64, 64)] if name == "many" else POOL_SHAPES):
        tg = torch.Generator().manual_seed(11 * sl.NAMES.index(name) + D + F)
        feats = torch.randn(N, D, generator=tg).to(torch.bfloat16).cuda()          # signed: a max of negative rows
        fsup = (torch.randn(N, D, generator=tg) * 3.0).to(torch.bfloat16).cuda()
        ZW = 2 * (F + D)
        Z = torch.full((P, ZW), float("nan"), device="cuda")
        rc = fn(_ptr(feats), _ptr(fsup), D, D, F, _ptr(seg_ptr), P, _ptr(Z), ZW, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        mx, mean, tol = er.pool_prepare_ref(feats, fsup, seg, P)
        tag = "pool %s D=%d F=%d" % (name, D, F)
        assert torch.equal(_bits(Z[:, :F]), torch.zeros(P, F, dtype=torch.int32, device="cuda")), tag + ": zero block"
        assert torch.equal(_bits(Z[:, F:F + D]), _bits(mx.float())), tag + ": maxima"
        assert bool(torch.isnan(Z[:, F + D:2 * F + D]).all()), tag + ": super output columns were written"
        worst = max(worst, _check(tag + " mean", Z[:, 2 * F + D:], mean, tol))
    print("worst pool_prepare %s %.3f" % (name, worst))


# ---------------------------------------------------------------------------------------------
# node side of the layers > 0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [False, True], ids=["ld64", "slot_of_128"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_node_uv_vs_fp64(N, slot):
    C = 64
    tg = torch.Generator().manual_seed(13 * N + slot)
    ld = 128 if slot else 64
    fbuf = torch.randn(N, ld, generator=tg).to(torch.bfloat16).cuda()
    sbuf = torch.randn(N, ld, generator=tg).to(torch.bfloat16).cuda()
    off = 64 if slot else 0
    f_in, s_in = fbuf[:, off:off + C], sbuf[:, off:off + C]
    Wuv, Wr, Wn = ((torch.randn(n, C, generator=tg) / 8).to(torch.bfloat16).cuda() for n in (2 * C, C, C))
    _, us, ut = (v.cuda() for v in er.bn_vectors(2 * C, tg))
    bn, sn, tn = (v.cuda() for v in er.bn_vectors(C, tg))
    br = (torch.randn(C, generator=tg) * 0.1).cuda()
    fn = _fn("yolat_debug_node_uv_eval_bf16", [P_, I64, P_, I64, I64] + [P_] * 9 + [P_, P_, P_, I64, P_])

    def run():
        UV = torch.full((N, 2 * C), float("nan"), dtype=torch.bfloat16, device="cuda")
        root = torch.full((N, C), float("nan"), device="cuda")
        so = torch.full((N, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
        rc = fn(_ptr(f_in), ld, _ptr(s_in), ld, N, _ptr(Wuv), _ptr(Wr), _ptr(Wn), _ptr(us), _ptr(ut), _ptr(br), _ptr(bn),
                _ptr(sn), _ptr(tn), _ptr(UV), _ptr(root), _ptr(so[:, off:]), ld, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return UV, root, so

    UV, root, so = run()
    for a, b in zip((UV, root, so), run()):
        assert torch.equal(_bits(a), _bits(b)), "two runs differ"
    tag = "node N=%d ld=%d" % (N, ld)
    f64, s64 = er.widen(f_in), er.widen(s_in)
    want, delta = er.stage_ref(f64, er.widen(Wuv), "tile", None, us, ut, relu=False)
    r = [_check(tag + " UV", UV, want, store_envelope(want, delta))]
    want, delta = er.stage_ref(f64, er.widen(Wr), "tile", br, None, None, relu=False)
    r.append(_check(tag + " root", root, want, delta))
    want, delta = er.stage_ref(s64, er.widen(Wn), "tile", bn, sn, tn, relu=True)
    r.append(_check(tag + " s_out", so[:, off:off + C], want, store_envelope(want, delta)))
    assert float(so[:, off + 2:off + C:16].float().abs().max()) == 0.0            # closed columns
    if slot:
        assert bool(torch.isnan(so[:, :off].float()).all()), tag + ": the slot's neighbour was written"
    print("worst node_uv N=%d %.3f" % (N, max(r)))


# ---------------------------------------------------------------------------------------------
# the classifier's GEMM
# ---------------------------------------------------------------------------------------------
HGEMM = [P_, CI, I64, I64, I64, P_, I64, I64, P_, P_, P_, CI, P_, CI, I64, ctypes.POINTER(CI), P_]


def _hgemm_case(M, K, Nout, a_f32, y_bf16, bn, form):
    tg = torch.Generator().manual_seed(M + 3 * K + Nout)
    A = torch.relu(torch.randn(M, K, generator=tg)) + 0.3 * torch.rand(M, K, generator=tg)
    A = (A if a_f32 else A.to(torch.bfloat16)).cuda()
    W = (torch.randn(Nout, K, generator=tg) / K ** 0.5).to(torch.bfloat16).cuda()
    if bn:
        b, s, t = (v.cuda() for v in er.bn_vectors(Nout, tg))
    else:
        b, s, t = (torch.randn(Nout, generator=tg) * 0.1).cuda(), None, None
    fn = _fn("yolat_debug_hgemm_eval_bf16", HGEMM)

    def run():
        Y = torch.full((M, Nout), float("nan"), dtype=torch.bfloat16 if y_bf16 else torch.float32, device="cuda")
        tf = CI(-1)
        rc = fn(_ptr(A), int(a_f32), K, M, K, _ptr(W), K, Nout, _ptr(b), _ptr(s), _ptr(t), int(bn), _ptr(Y), int(y_bf16),
                Nout, ctypes.byref(tf), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return Y, tf.value

    Y, got_form = run()
    assert got_form == form, (M, K, Nout, got_form)
    assert torch.equal(_bits(Y), _bits(run()[0])), "two runs differ"
    want, delta = er.stage_ref(bf(A) if a_f32 else er.widen(A), er.widen(W), "tile", b, s, t, relu=bn)
    tag = "hgemm %s M=%d K=%d Nout=%d %s" % ("FOp" if a_f32 else "HOp", M, K, Nout, "bf16" if y_bf16 else "fp32")
    return _check(tag, Y, want, store_envelope(want, delta) if y_bf16 else delta)


MS = [1, 63, 64, 65, 400]


@pytest.mark.parametrize("K,Nout", [(2304, 512), (64, 64), (128, 64), (192, 256)])
@pytest.mark.parametrize("M", MS)
def test_hgemm_fp32_rows_bf16_out(M, K, Nout):
    _hgemm_case(M, K, Nout, True, True, True, 0)


@pytest.mark.parametrize("M", MS)
def test_hgemm_bf16_rows_bf16_out(M):
    _hgemm_case(M, 512, 256, False, True, True, 0)


@pytest.mark.parametrize("Nout", [17, 1])
@pytest.mark.parametrize("M", MS)
def test_hgemm_bf16_rows_fp32_logits_on_a_masked_tile(M, Nout):
    _hgemm_case(M, 256, Nout, False, False, False, 0)


@pytest.mark.parametrize("M", [4095, 4096])
def test_hgemm_64x128_tile_form(M):
    _hgemm_case(M, 128, 512, True, True, True, 1)
