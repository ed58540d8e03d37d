"""GPU tests: --act leakyrelu / prelu models on the bf16-STORAGE eval forward (set_eval_precision("bf16", leaky_act=True),
csrc/bf16_eval.hip + the ACT instantiation of fusion_h8.hip): forward, predict, detect_submit / evaluate_submit, hipGraph
replay, prepared-graph and DeviceLoader batches.

Bars are the project's bf16 bars (tests/test_gpu_bf16.py): max |logit error| <= RTOL_BF16 = 2e-2 of the largest reference
logit and rms error <= RMS_BF16 = 1e-2 of the logits' rms, against the fp32 CPU oracle — multiplied by the product of
max(1, |a_i|) over the four activation sites (the activation is max(1, |a|)-Lipschitz: an error entering a site leaves it
scaled by at most that), which is 1.4 for prelu_mixed and 1 for the other variants (prelu_filled, whose slopes fill_state_
draws from (0.5, 1.5), is held to the plain bars as well).

Measured on the MI355X (max of the scale / rms), worst shape per variant: leakyrelu 1.04e-2 / 7.6e-3 (d64), prelu_filled
7.6e-3 / 6.2e-3, prelu_neg 6.8e-3 / 5.0e-3, prelu_zero 8.5e-3 / 6.8e-3, prelu_mixed 1.34e-2 / 7.0e-3 (bars 2.8e-2 / 1.4e-2).

Variants and shapes are those of tests/test_gpu_act_model.py (p23: the skinny sizes; d64: fusion_dims 64; p1100: more than
1024 proposals, where the one-launch conv stack writes the zero block that yolat_pool_init_signed then overwrites), plus
b3: n_blocks_out = 3, D = 192, the materialising fusion route.
"""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import golden_util as gu
import test_gpu_act_model as am
from oracle import oracle_torch as orc

pytestmark = pytest.mark.gpu

RTOL_BF16 = 2e-2        # max |logit error| / max |logit|          (tests/test_gpu_bf16.py)
RMS_BF16 = 1e-2         # rms error / rms logit

SHAPES = {k: am.SHAPES[k] for k in ("p23", "d64", "p1100")}
SHAPES["b3"] = (dict(n_blocks=3, n_blocks_out=3), dict(num_proposals=40, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=60))


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _optkw(variant, shape, **more):
    kw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, act=am.VARIANTS[variant][0] if variant != "relu" else "relu")
    kw.update(SHAPES[shape][0])
    kw.update(more)
    return kw


def _build(cls_mod, variant, shape, seed=31):
    model = gu.fill_state_(cls_mod.SparseCADGCN(cls_mod.Opt(**_optkw(variant, shape))), seed)
    return am._set_slopes(model, am.VARIANTS[variant][1]) if variant != "relu" else model


@functools.lru_cache(maxsize=None)
def _graph(shape):
    kw = SHAPES[shape][1]
    return am._tiny_proposals(**kw) if kw["nodes_lo"] == 1 else _yv().synth_graph(n_classes=17, **kw)


@functools.lru_cache(maxsize=None)
def _oracle(variant, shape):
    """(fp32 CPU oracle logits, bar factor) — computed once per case, read only"""
    ref = _build(orc, variant, shape).eval()
    with torch.no_grad():
        logits = ref(_graph(shape), None)[0]
    factor = 1.0
    for a in (am.VARIANTS[variant][1] if variant != "relu" else None) or ():
        factor *= max(1.0, abs(a))
    return logits, factor


def _bf16_model(variant, shape):
    return _build(_yv(), variant, shape).cuda().eval().set_eval_precision("bf16", leaky_act=True)


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.double()
    return (float((got - want).abs().max()) / float(want.abs().max()),
            float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()))


def _within_bars(name, got, want, factor):
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
    mx, rms = _rel(got, want)
    print("bf16 %s: max %.3e (bar %.3e)  rms %.3e (bar %.3e)" % (name, mx, RTOL_BF16 * factor, rms, RMS_BF16 * factor))
    assert mx <= RTOL_BF16 * factor, "%s: max error %.3e of the logits' scale" % (name, mx)
    assert rms <= RMS_BF16 * factor, "%s: rms error %.3e of the logits' rms" % (name, rms)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("variant", list(am.VARIANTS))
def test_bf16_eval_forward_matches_the_fp32_oracle(variant, shape):
    want, factor = _oracle(variant, shape)
    model = _bf16_model(variant, shape)
    d = _graph(shape)
    with torch.no_grad():
        got = model(d, None)[0]
        again = model(d, None)[0]
    model.check_last_status()
    _within_bars("%s %s" % (variant, shape), got, want, factor)
    assert torch.equal(got, again)                                    # two forwards: the same bits
    assert model._yolat_plan.precision == "bf16" and model._yolat_plan._desc.act != 0


def test_the_leaky_bf16_model_is_not_the_relu_bf16_model():
    """a forward that ignored the activation would sit within the bar of the wrong model"""
    want, _ = _oracle("leakyrelu", "p23")
    d = _graph("p23")
    with torch.no_grad():
        leaky = _bf16_model("leakyrelu", "p23")(d, None)[0]
        relu = _bf16_model("relu", "p23")(d, None)[0]
    mx, _ = _rel(relu, want)
    assert mx > 2 * RTOL_BF16
    _within_bars("leakyrelu p23", leaky, want, 1.0)


@pytest.mark.parametrize("shape", ["p23", "b3"])
@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "hipgraph"])
def test_in_place_slope_edit_is_seen_by_the_next_forward(graphs, shape):
    yv = _yv()
    model = _bf16_model("prelu_filled", shape)
    d = _graph(shape)
    dd = yv.Data(x=d.x.cuda(), pos=d.pos)
    for k in ("edge", "e_attr", "bbox_idx", "bbox"):
        dd[k] = d[k].cuda()
    model.use_hip_graphs(graphs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), torch.no_grad():
        first = [model(dd, None)[0] for _ in range(3)]                # direct, capture, replay
        plan = model._yolat_plans[s.cuda_stream]
        build = plan._desc_key
        am._set_slopes(model, (-0.3,) * 4)
        after = [model(dd, None)[0] for _ in range(2)]
    torch.cuda.synchronize()
    assert plan._desc_key == build                                    # the slopes are not part of the weight version
    if graphs:
        assert any(v not in (False, None) for v in plan._graphs.values())      # the captured graph survived the edit
    (want0, f0), (want1, f1) = _oracle("prelu_filled", shape), _oracle("prelu_neg", shape)
    for o in first:
        _within_bars("before the edit", o, want0, f0)
    for o in after:
        _within_bars("after the edit", o, want1, f1)
    assert torch.equal(first[0], first[2]) and torch.equal(after[0], after[1])
    assert _rel(first[0], want1)[0] > 2 * RTOL_BF16                   # the edit matters at these bars


def _ws_bytes(plan, N, E, P):
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    return int(lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(plan._desc_h), N, E, P))


@pytest.mark.parametrize("shape", ["p23", "b3"])
def test_relu_bf16_forward_and_workspace_do_not_move_when_a_leaky_model_is_planned(shape):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import ops
    d = _graph(shape)
    relu = _bf16_model("relu", shape)
    with torch.no_grad():
        before = relu(d, None)[0].clone()
    st = relu._stage_tensors(d)
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E = ops.edge_layout(st["edge"])[0]
    assert relu._yolat_plan._desc.act == 0 and all(not p for p in relu._yolat_plan._desc.act_slope)
    need = _ws_bytes(relu._yolat_plan, N, E, P)
    leaky = _bf16_model("prelu_neg", shape)
    with torch.no_grad():
        leaky(d, None)
        after = relu(d, None)[0]
        fresh = _bf16_model("relu", shape)(d, None)[0]
    assert torch.equal(before, after) and torch.equal(before, fresh)
    assert _ws_bytes(relu._yolat_plan, N, E, P) == need
    need_leaky = _ws_bytes(leaky._yolat_plan, N, E, P)
    if shape == "p23":
        assert need_leaky == need              # the rows kernel needs no scratch beyond the ReLU forward's
    else:
        # the materialising route: one column range of the fusion block's BatchNorm output in fp32, carved last
        F = relu._yolat_plan._desc.F
        assert need < need_leaky <= need + 4 * N * F + 512


@pytest.mark.parametrize("variant", ["leakyrelu", "prelu_neg"])
def test_prepared_graph_and_device_loader_batches_equal_the_plain_forward(variant):
    yv = _yv()
    model = _bf16_model(variant, "p23")
    d = _graph("p23")
    with torch.no_grad():
        want = model(d, None)[0]
        b, sl = yv.collate_to_device([d], csr=True)
        got_csr = model(b, sl)[0]
        b2, sl2 = yv.collate_to_device([d])
        got_coo = model(b2, sl2)[0]
        loader = yv.DeviceLoader([[d], [d]], slots=2)
        got_loader = [model(bb, ss)[0].clone() for bb, ss in loader]
        loader.close()
    ref, factor = _oracle(variant, "p23")
    _within_bars("plain", want, ref, factor)
    assert torch.equal(got_coo, want)
    # (the bf16 forward runs the same launches on a prepared graph's arrays: bits, not a bar)
    assert torch.equal(got_csr, want)
    assert len(got_loader) == 2 and all(torch.equal(o, want) for o in got_loader)


def _predict_both(yv, model, data, slices):
    from yolat_vectorgraphicsrecognition_amd import architecture as A
    calls = []
    orig = model._predict_two_pass
    model._predict_two_pass = lambda d, s: calls.append(1) or orig(d, s)
    try:
        with torch.no_grad():
            A.PREDICT_ONE_SUBMISSION = True
            one = model.predict(data, slices)
            assert calls == []                                        # the one-submission path took the call
            A.PREDICT_ONE_SUBMISSION = False
            try:
                two = model.predict(data, slices)
            finally:
                A.PREDICT_ONE_SUBMISSION = True
            assert calls == [1]
    finally:
        del model._predict_two_pass
    return one, two


def test_predict_both_ways():
    yv = _yv()
    data, slices = yv.synth_batch(2, 21, num_proposals=300, nodes_lo=4, nodes_hi=30, edge_factor=1.3, with_roots=True)
    kw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, act="prelu")
    model = am._set_slopes(gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 3), (-0.3,) * 4).cuda().eval()
    model.set_eval_precision("bf16", leaky_act=True)
    with torch.no_grad():                 # "has object" the arg-max of about half of the proposals: the child pass has work
        z = model(data, slices)[0]
        gap = z[:, :-1].max(1).values - z[:, -1]
        model.prediction_cls[2][0].bias[model.n_classes - 1] += float(gap.median())
    data._yolat_stage = None
    one, two = _predict_both(yv, model, data, slices)
    assert one[2] is None and one[5] is None
    np.testing.assert_array_equal(np.array([int(v) for v in one[3]]), np.array([int(v) for v in two[3]]))
    assert [int(v) for v in one[4]] == [int(v) for v in two[4]]
    assert len(data.roots) < len(one[3]) < data.bbox.shape[0] + 1
    assert torch.equal(one[1], two[1])
    assert one[0].shape == two[0].shape and one[0].is_cuda
    assert float((one[0] - two[0]).abs().max()) <= RTOL_BF16 * float(two[0].abs().max())
    # ... and the fp32 CPU oracle's logits on the rows both selected
    ref = am._set_slopes(gu.fill_state_(orc.SparseCADGCN(orc.Opt(**kw)), 3), (-0.3,) * 4).eval()
    with torch.no_grad():
        ref.prediction_cls[2][0].bias.copy_(model.prediction_cls[2][0].bias.cpu())
        full = ref(data, slices)[0]
    rows = [int(v) for v in one[3]]
    _within_bars("predict rows", one[0], full[rows], 1.0)


def _leaky_predict_model(yv, classifier="softmax"):
    kw = dict(gu.PREDICT_OPT, act="leakyrelu", classifier=classifier)
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 5).cuda().eval().set_eval_precision("bf16", leaky_act=True)


def test_detect_submit_equals_detect_batch():
    from test_gpu_detect import _eval_loader
    from test_gpu_detect_async import _same
    yv = _yv()
    model = _leaky_predict_model(yv)
    batch = _eval_loader(yv, 6)[1]
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5).result()
    _same(got, want)
    assert sum(g.shape[0] for g in got) > 0
    data, slices = copy.deepcopy(batch)
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same(model.detect_submit(data, slices, conf_thres=0.05, iou_thres=0.5).result(), want)


def test_evaluate_submit_equals_evaluate_batch():
    from test_gpu_detect import _eval_loader
    from test_gpu_evaluate_async import _same_rep, _sync
    yv = _yv()
    model = _leaky_predict_model(yv)
    K = gu.PREDICT_OPT["n_classes"]
    loader = _eval_loader(yv, 4)
    for batch in loader:
        want = _sync(yv, model, copy.deepcopy(batch))
        got = yv.evaluate_batch_async(model, *copy.deepcopy(batch)).result()
        _same_rep(got, want, K)
        assert got["n_total"] > 0 and math.isfinite(got["loss"]["loss"])
    data, slices = copy.deepcopy(loader[1])
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same_rep(model.evaluate_submit(data, slices).result(), want, K)


def test_detect_stream_and_evaluate_stream():
    from test_gpu_detect_async import _loader_lists, _same
    from test_gpu_evaluate_async import _same_rep, _stream_lists, _sync
    yv = _yv()
    K = 17
    kw = dict(n_classes=K, n_blocks=2, n_blocks_out=2, act="prelu")
    model = am._set_slopes(gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 13), (-0.3,) * 4).cuda().eval()
    model.set_eval_precision("bf16", leaky_act=True)
    opts = dict(conf_thres=0.05, iou_thres=0.5)
    lists = _loader_lists(yv, 3)
    want = [yv.detect_batch(model, *yv.collate_to_device(items), fixup=False, **opts) for items in lists]
    got = list(yv.detect_stream(model, [yv.collate_to_device(items) for items in lists], depth=2, **opts))
    assert len(got) == 3
    for g, w in zip(got, want):
        _same(g, w)
    lists = _stream_lists(yv, 3, K)
    want = [_sync(yv, model, yv.collate_to_device(copy.deepcopy(items)), fixup=False) for items in lists]
    loader = yv.DeviceLoader(copy.deepcopy(lists), slots=4, csr=False)
    got = list(yv.evaluate_stream(model, loader, depth=2))
    loader.close()
    assert len(got) == 3 and sum(w["n_total"] for w in want) > 0
    for g, w in zip(got, want):
        _same_rep(g, w, K)


def test_still_loud():
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd.plan import EvalPlan
    with pytest.raises(ValueError, match="norm"):
        yv.SparseCADGCN(yv.Opt(norm="layer")).set_eval_precision("bf16")
    with pytest.raises(ValueError, match="norm"):
        EvalPlan(yv.SparseCADGCN(yv.Opt(norm="layer")).cuda(), "bf16")
    with pytest.raises(NotImplementedError):
        yv.SparseCADGCN(yv.Opt(act="leakyrelu", norm="layer"))
    for act in ("leakyrelu", "prelu"):
        m = yv.SparseCADGCN(yv.Opt(act=act))
        with pytest.raises(ValueError, match="leaky_act"):      # the plain call declines as it always did, and says how
            m.set_eval_precision("bf16")
        assert m.set_eval_precision("bf16", leaky_act=True) is m and m.set_eval_precision("fp32") is m
        for prec in ("bf16", "bf16_dense"):
            with pytest.raises(ValueError, match="act"):
                m.set_train_precision(prec)


@pytest.mark.parametrize("how", ["act3", "null_slope"])
def test_c_abi_declines_a_bad_activation_before_any_launch(how):
    """yolat_forward_eval_bf16 on a descriptor with act = 3, or act = 1 and a NULL slope: YOLAT_E_INVALID, the logits
    and the status word untouched"""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    model = _bf16_model("leakyrelu", "p23")
    d = _graph("p23")
    with torch.no_grad():
        good = model(d, None)[0]
    plan = model._yolat_plan
    st = model._stage_tensors(d)
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E, se, sc = ops.edge_layout(st["edge"])
    ws = torch.zeros(_ws_bytes(plan, N, E, P) + 256, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((P, 17), float("nan"), device="cuda")

    def call():
        rc = lib.yolat_forward_eval_bf16(ctypes.byref(plan._desc_h), st["x"].data_ptr(), st["x"].stride(0),
                                         st["edge"].data_ptr(), se, sc, st["e_attr"].data_ptr(), st["bbox_idx"].data_ptr(),
                                         N, E, P, out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
                                         status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    assert call() == 0 and torch.equal(out, good)                     # the hand-made call itself is sound
    out.fill_(float("nan"))
    ws.zero_()
    saved = (plan._desc.act, plan._desc.act_slope[2])
    try:
        if how == "act3":
            plan._desc.act = 3
        else:
            plan._desc.act, plan._desc.act_slope[2] = 1, None
        assert call() == -1                                           # YOLAT_E_INVALID
        assert lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(plan._desc_h), N, E, P) > 0
    finally:
        plan._desc.act, plan._desc.act_slope[2] = saved
    assert bool(torch.isnan(out).all()) and int(status.item()) == 0 and int(ws.count_nonzero()) == 0
    assert call() == 0 and torch.equal(out, good)
