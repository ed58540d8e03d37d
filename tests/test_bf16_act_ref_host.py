"""CPU test (-m "not gpu") of the claims of tests/bf16_act_ref.py, the float64 model the leaky bf16 stages are held to:

  * a literal fp32 evaluation of every stage (bf16 operands widened, fp32 matmul, fp32 epilogue, act(y) = y > 0 ? y : a y
    in fp32, amax of the activated rows, one rounding to bf16 where the stage stores bf16) lies inside the envelope
    max(1, |a|) delta + 2^-24 |a val| for the slopes 0.2, -0.3, 1.4 and 0, in the fold and the tile form;
  * the envelope rejects the wrong kernels: activation AFTER the maximum (a = -0.3), ReLU in place of the activation, the
    two slopes swapped, and a bf16 store of the pre-activation followed by the activation (two roundings);
  * the inputs of the GPU test reach what the signed pooling is for, on the reference itself: for every layout of
    segmax_layouts.NAMES at least 2 % of the pooled entries are negative for a = 0.2, and for a = -0.3 at least 5 % of the
    entries of the proposals with two or more rows differ from act(max pre) (`many` has one-row proposals only, where the
    two are the same number: there the share is asserted to be exactly 0 and the layout still runs on the GPU)."""
import pytest
import torch

import bf16_act_ref as ar
import bf16_eval_ref as er
import segmax_layouts as sl
from bf16_ref import store_envelope


def _inside(got, want, tol):
    return (got.double() - want).abs() <= tol


@pytest.mark.parametrize("a", ar.SLOPES)
@pytest.mark.parametrize("name", ["straddle", "tiny_then_long", "empty", "small_n33"])
def test_fp32_evaluation_of_the_pooled_stage_is_inside_the_envelope(name, a):
    lay = sl.layout(name)
    inp = ar.fusion_act_inputs(lay, 64, 128)
    seg = er.seg_tensor(lay)
    a64 = ar.slope64(a)
    for form, W, b, s, t in (("fold", inp["Wfold"], None, None, inp["tfold"]), ("tile", inp["W"], inp["b"], inp["s"], inp["t"])):
        val32 = er.emulate_stage(inp["feats"], W, form, b, s, t, relu=False)
        got = ar.emulate_pool_act(ar.emulate_act(val32, a), seg, lay.P)
        want, tol, _ = ar.fusion_pool_act_ref(inp["feats"], W, form, b, s, t, seg, lay.P, a64)
        assert bool(_inside(got, want, tol).all()), (name, a, form)
        empty = torch.from_numpy(lay.sizes == 0)
        assert float(want[empty].abs().sum()) == 0.0


@pytest.mark.parametrize("a", ar.SLOPES)
def test_fp32_evaluation_of_the_stored_stage_is_inside_the_envelope(a):
    tg = torch.Generator().manual_seed(5)
    A = torch.randn(65, 512, generator=tg)
    W = (torch.randn(256, 512, generator=tg) / 512 ** 0.5).to(torch.bfloat16)
    b, s, t = er.bn_vectors(256, tg)
    a64 = ar.slope64(a)
    val32 = er.emulate_stage(A.to(torch.bfloat16), W, "tile", b, s, t, relu=False)
    got = ar.emulate_act(val32, a).to(torch.bfloat16)
    want, env = ar.super_act_ref(A, W, "tile", b, s, t, a64)
    assert bool(_inside(got, want, store_envelope(want, env)).all())
    if a != 0.0:
        # two roundings (the pre-activation stored as bf16, then activated and stored again) are not the contract
        twice = ar.emulate_act(val32.to(torch.bfloat16).float(), a).to(torch.bfloat16)
        assert int((~_inside(twice, want, store_envelope(want, env))).sum()) > 0


def test_envelope_rejects_the_wrong_kernels():
    lay = sl.layout("straddle")
    inp = ar.fusion_act_inputs(lay, 64, 128)
    seg = er.seg_tensor(lay)
    a = ar.slope64(-0.3)
    val32 = er.emulate_stage(inp["feats"], inp["Wfold"], "fold", None, None, inp["tfold"], relu=False)
    want, tol, _ = ar.fusion_pool_act_ref(inp["feats"], inp["Wfold"], "fold", None, None, inp["tfold"], seg, lay.P, a)
    pre_max = ar.emulate_pool_act(val32, seg, lay.P)
    after = ar.emulate_act(pre_max, -0.3)                                  # activation after the maximum
    assert float((~_inside(after, want, tol)).double().mean()) > 0.05
    relu = ar.emulate_pool_act(torch.relu(val32), seg, lay.P)              # the ReLU kernel
    assert float((~_inside(relu, want, tol)).double().mean()) > 0.02
    other = ar.emulate_pool_act(ar.emulate_act(val32, 0.2), seg, lay.P)    # the other problem's slope
    assert float((~_inside(other, want, tol)).double().mean()) > 0.05


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", sl.NAMES)
def test_inputs_of_the_gpu_cases_exercise_the_signed_pooling(name, D):
    lay = sl.layout(name)
    inp = ar.fusion_act_inputs(lay, D, 128)
    seg = er.seg_tensor(lay)
    args = (inp["feats"], inp["Wfold"], "fold", None, None, inp["tfold"], seg, lay.P)
    want, _, aom = ar.fusion_pool_act_ref(*args, ar.slope64(0.2))
    neg, _, _ = ar.exercise(want, aom, seg, lay.P)
    want, _, aom = ar.fusion_pool_act_ref(*args, ar.slope64(-0.3))
    _, differ, multi = ar.exercise(want, aom, seg, lay.P)
    print("exercise %-16s D=%d negative %.3f differ %.3f multi-row proposals %d" % (name, D, neg, differ, multi))
    assert neg >= 0.02
    if multi:
        assert differ >= 0.05
    else:
        assert name == "many" and differ == 0.0
