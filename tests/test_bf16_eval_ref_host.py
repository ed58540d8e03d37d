"""CPU test (-m "not gpu") of tests/bf16_eval_ref.py, the float64 model and envelope that tests/test_gpu_bf16_eval_stages.py
holds the dense stages of the bf16-storage eval forward to.  On the `straddle`, `tiny_then_long` and `empty` layouts:

  1. an fp32 emulation of every stage (bf16 operands, torch fp32 matmul, fp32 epilogue; bf16_eval_ref.emulate_stage) stays
     inside the envelope at every element: the fusion pair in its three epilogue forms at D = 128 and D = 192, the super
     block, the pooling prologue, the node side and the classifier's GEMM;
  2. each of these wrong kernels leaves it in at least one element (the bound is tight enough to matter):
       drop_row      the last row before a 256-row edge is missing from its proposal's max
       credit_prev   the row after a 256-row edge is credited to the previous proposal
       trunc_input   the super block's fp32 input truncated to bf16 instead of rounded
       short_k       the last 8 k-columns of A ignored
       stale_shift   column tile j + 1 computed with column tile j's shift
       lds_garbage   D = 192: columns 192..255 of the LDS image not zeroed (garbage x the clamped weight chunk)
       trunc_store   a bf16 output stored by truncation
       odd_k_step    the classifier GEMM without its last 64-wide K step when K / 64 is odd
     The two row mutations need an edge that separates two proposals, and a proposal that is not filled with copies of one
     row: on `straddle` that is row 255 | 256, on `tiny_then_long` 511 | 512.  `empty` has one 256-row edge, inside a
     200-row proposal that tie_proposals fills: there drop_row runs on inputs without the tie fill and with row 255
     doubled (exact in bf16), so that the row holds its proposal's maximum in many columns, and credit_prev does not
     change the computation (asserted).  Every other mutation is rejected on all three layouts.
"""
import numpy as np
import pytest
import torch

import bf16_eval_ref as er
import segmax_layouts as sl
from bf16_ref import EPS32, bf, store_envelope, truncate_bf16, ulp_bf16

LAYOUTS = ("straddle", "tiny_then_long", "empty")
F = 192
EDGE = {"straddle": 256, "tiny_then_long": 512, "empty": 256}
FORM_W = {"fold": ("Wfold", None, None, "tfold"), "rows": ("W", "b", "s", "t"), "tile": ("W", "b", "s", "t")}


def _inside(name, got, want, tol):
    ratio, bad = er.worst(name, got, want, tol)
    assert bad == 0, (name, bad, ratio)
    return ratio


def _outside(name, got, want, tol):
    ratio, bad = er.worst(name, got, want, tol)
    assert bad >= 1, (name, "a wrong kernel stays inside the envelope", ratio)


def _args(inp, form, k=""):
    w, b, s, t = FORM_W[form]
    return inp[w + k], (inp[b + k] if b else None), (inp[s + k] if s else None), inp[t + k]


def _pooled(inp, lay, form, seg, acc=None, t=None, seg_used=None):
    w, b, s, t0 = _args(inp, form)
    val = er.emulate_stage(inp["feats"], w, form, b, s, t0 if t is None else t, acc=acc)
    return er.emulate_pool(val, seg if seg_used is None else seg_used, lay.P)


@pytest.mark.parametrize("D", [128, 192])
@pytest.mark.parametrize("name", LAYOUTS)
def test_fusion_pair_emulation_inside_and_wrong_kernels_outside(name, D):
    lay = sl.layout(name)
    seg = er.seg_tensor(lay)
    inp = er.fusion_inputs(lay, D, F, 100 * LAYOUTS.index(name) + D)
    edge = EDGE[name]
    for form in er.FORMS:
        w, b, s, t = _args(inp, form)
        want, tol = er.fusion_pool_ref(inp["feats"], w, form, b, s, t, seg, lay.P)
        tag = "%s D=%d %s" % (name, D, form)
        _inside(tag + " pooled", _pooled(inp, lay, form, seg), want, tol)
        empty = torch.from_numpy(lay.sizes == 0)
        assert float(want[empty].abs().max()) == 0.0 if bool(empty.any()) else True
        assert float(want[:, 2::16].abs().max()) == 0.0                       # closed columns
        assert float(want[~empty][:, 0::16].min()) > 0.0                      # s == +-0 columns hold t > 0
        # short_k / stale_shift / lds_garbage: independent of the layout
        a32, w32 = inp["feats"].float(), w.float()
        _outside(tag + " short_k", _pooled(inp, lay, form, seg, acc=a32[:, :-8] @ w32[:, :-8].t()), want, tol)
        ts = t.clone()
        ts[64:128] = t[0:64]
        _outside(tag + " stale_shift", _pooled(inp, lay, form, seg, t=ts), want, tol)
        if D == 192:
            tg = torch.Generator().manual_seed(5)
            garbage = torch.randn(lay.N, 64, generator=tg).to(torch.bfloat16).float()
            acc = a32 @ w32.t() + garbage @ w32[:, 184:192].repeat(1, 8).t()   # the loads clamp k to K - 8
            _outside(tag + " lds_garbage", _pooled(inp, lay, form, seg, acc=acc), want, tol)
        # credit_prev: the row after the edge carries the id of the row before it
        moved = seg.clone()
        moved[edge] = seg[edge - 1]
        if name == "empty":
            assert int(seg[edge]) == int(seg[edge - 1])                        # one proposal across the only edge
        else:
            assert int(seg[edge]) != int(seg[edge - 1])
            _outside(tag + " credit_prev", _pooled(inp, lay, form, seg, seg_used=moved), want, tol)
        # drop_row: the row before the edge takes no part in the max (a row id no proposal has: dropped by the scatter)
        inp_d, want_d, tol_d = inp, want, tol
        if name == "empty":
            inp_d = er.fusion_inputs(lay, D, F, 100 * LAYOUTS.index(name) + D, ties=False)
            inp_d["feats"][edge - 1] = (inp_d["feats"][edge - 1].float() * 2.0).to(torch.bfloat16)
            w, b, s, t = _args(inp_d, form)
            want_d, tol_d = er.fusion_pool_ref(inp_d["feats"], w, form, b, s, t, seg, lay.P)
            _inside(tag + " pooled (no tie fill)", _pooled(inp_d, lay, form, seg), want_d, tol_d)
        else:
            assert int(seg[edge - 1]) not in sl.tie_proposals(lay)
        w, b, s, t = _args(inp_d, form)
        val = er.emulate_stage(inp_d["feats"], w, form, b, s, t)
        keep = torch.ones(lay.N, dtype=torch.bool)
        keep[edge - 1] = False
        got = er.emulate_pool(val[keep], seg[keep], lay.P)
        _outside(tag + " drop_row", got, want_d, tol_d)
    # the super block: fp32 rows rounded to nearest even while loading (fold and tile forms)
    for form in ("fold", "tile"):
        w, b, s, t = _args(inp, form, "s")
        want, tol = er.super_ref(inp["S"], w, form, b, s, t)
        tag = "%s D=%d super %s" % (name, D, form)
        _inside(tag, er.emulate_stage(inp["S"].to(torch.bfloat16), w, form, b, s, t), want, tol)
        _outside(tag + " trunc_input", er.emulate_stage(truncate_bf16(inp["S"]), w, form, b, s, t), want, tol)


@pytest.mark.parametrize("name", LAYOUTS)
def test_pool_prologue_emulation_inside(name):
    lay = sl.layout(name)
    seg = er.seg_tensor(lay)
    tg = torch.Generator().manual_seed(3 + LAYOUTS.index(name))
    feats = torch.randn(lay.N, 64, generator=tg).to(torch.bfloat16)
    fsup = (torch.randn(lay.N, 64, generator=tg) * 3.0).to(torch.bfloat16)
    mx, mean, tol = er.pool_prepare_ref(feats, fsup, seg, lay.P)
    cnt = torch.from_numpy(lay.sizes)
    # fp32, one row after the other (index_add_ on the CPU walks the rows in order), one division
    sm32 = torch.zeros(lay.P, 64).index_add_(0, seg, fsup.float())
    _inside(name + " mean", sm32 / cnt.clamp_min(1).float()[:, None], mean, tol)
    assert float(mx[cnt == 0].abs().max()) == 0.0 if bool((cnt == 0).any()) else True
    assert float(mx[cnt > 0].min()) < 0.0                                      # a max of negative rows is negative, not 0
    # a sum that loses its last row is outside
    last = torch.from_numpy(sl.starts(lay) + lay.sizes - 1)[cnt > 1]
    sm_bad = sm32.clone()
    sm_bad[cnt > 1] -= fsup.float()[last]
    _outside(name + " mean without the last row", sm_bad / cnt.clamp_min(1).float()[:, None], mean, tol)


@pytest.mark.parametrize("M", [1, 65, 400])
def test_node_side_and_classifier_emulation_inside_and_wrong_stores_outside(M):
    tg = torch.Generator().manual_seed(M)
    # node side: UV = dot s + t (bf16), root = dot + b (fp32), s_out = relu((dot + b) s + t) (bf16)
    f = torch.randn(M, 64, generator=tg).to(torch.bfloat16)
    Wuv = (torch.randn(128, 64, generator=tg) / 8).to(torch.bfloat16)
    _, s, t = er.bn_vectors(128, tg)
    want, delta = er.stage_ref(er.widen(f), er.widen(Wuv), "tile", None, s, t, relu=False)
    val = er.emulate_stage(f, Wuv, "tile", None, s, t, relu=False)
    _inside("UV M=%d" % M, val.to(torch.bfloat16), want, store_envelope(want, delta))
    _outside("UV M=%d trunc_store" % M, truncate_bf16(val), want, store_envelope(want, delta))
    Wr = (torch.randn(64, 64, generator=tg) / 8).to(torch.bfloat16)
    br = torch.randn(64, generator=tg) * 0.1
    want, delta = er.stage_ref(er.widen(f), er.widen(Wr), "tile", br, None, None, relu=False)
    _inside("root M=%d" % M, er.emulate_stage(f, Wr, "tile", br, relu=False), want, delta)
    # classifier: fp32 rows rounded while staging, K = 2304 and K = 192 (K / 64 odd), folded BatchNorm + ReLU, bf16 out
    for K, Nout in ((2304, 512), (192, 256)):
        A = torch.relu(torch.randn(M, K, generator=tg)) + 0.3 * torch.rand(M, K, generator=tg)
        W = (torch.randn(Nout, K, generator=tg) / K ** 0.5).to(torch.bfloat16)
        b, s, t = er.bn_vectors(Nout, tg)
        want, delta = er.stage_ref(bf(A), er.widen(W), "tile", b, s, t)
        env = store_envelope(want, delta)
        tag = "cls M=%d K=%d" % (M, K)
        val = er.emulate_stage(A.to(torch.bfloat16), W, "tile", b, s, t)
        _inside(tag, val.to(torch.bfloat16), want, env)
        _outside(tag + " trunc_store", truncate_bf16(val), want, env)
        _outside(tag + " trunc_input", er.emulate_stage(truncate_bf16(A), W, "tile", b, s, t).to(torch.bfloat16), want, env)
        if (K // 64) % 2 == 1:
            acc = A.to(torch.bfloat16).float()[:, :K - 64] @ W.float()[:, :K - 64].t()
            _outside(tag + " odd_k_step", er.emulate_stage(None, W, "tile", b, s, t, acc=acc).to(torch.bfloat16), want, env)


def test_planners_give_the_splits_the_gpu_cases_are_written_for():
    """the (groups, ng) the GPU test asserts come from these restatements of the host planners"""
    assert er.plan_h8(1100, 1024) == (16, 1)
    assert [er.plan_h8(1100, 1024, g) for g in (1, 3, 8)] == [(1, 16), (3, 6), (8, 2)]
    assert er.plan_h8(1100, 960, 2) == (2, 8)
    assert er.plan_h8(66000, 1024) == (1, 16)
    assert er.plan_rows(1100, 160, 1) == (1, 3) and er.plan_rows(1100, 160, 4) == (3, 1)
    assert er.plan_rows(1100, 1024) == (16, 1) and er.plan_rows(1100, 1024, 1) == (1, 16)
    assert er.plan_rows(8192 + 37, 1024) == (8, 2)


def test_rounding_helpers_agree_with_torch():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    assert torch.equal(bf(x), x.to(torch.bfloat16).double())
    tr = truncate_bf16(x).double()
    assert bool(((tr - x.double()).abs() < ulp_bf16(x)).all()) and bool((tr.abs() <= x.double().abs()).all())
    assert int((tr != bf(x)).sum()) > 1000
    assert np.isclose(float(EPS32), 2.0 ** -24)
