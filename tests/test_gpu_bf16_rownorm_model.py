"""GPU tests: --norm layer / instance models on the bf16-STORAGE eval forward (set_eval_precision("bf16", row_norm=True);
csrc/fusion_h8_rn.hip + the row-norm branches of csrc/bf16_eval.hip): forward on both fusion routes, predict,
evaluate_batch / evaluate_submit, in-place edits of gamma, and the norm = batch bf16 forward pinned to the parent commit.

Reference: the SAME model's fp32 HIP forward (pinned to the oracle at 1e-4 by tests/test_gpu_norm_model.py).  Bars: the
project's standing bf16 contract (max <= 1.5e-2 of the logits' scale, rms <= 1e-2 of their rms) — the gap
measured for row-norm models is INSIDE it (profiles/bf16_rownorm_contract.txt, tools/bf16_rownorm_ab.py --contract), so the
standing bars are asserted, not the measured maximum times two: MEASURED_MAX below is kept next to them as the record, and
the test also holds the gap to 2 x MEASURED_MAX wherever that is the tighter of the two.  Arg-max agreement >= 0.99 is
asserted where there are enough rows for the figure to mean something (P >= 1000).

Measured on the MI355X, these graphs (max / rms / agreement): layer p23 6.3e-3 / 3.7e-3 / 1, d64 9.5e-3 / 7.2e-3 / 1, p1100
7.1e-3 / 3.9e-3 / 0.9900 (fused) and 0.9918 (materialising), b3 4.8e-3 / 3.3e-3 / 1; instance p23 7.2e-3 / 4.5e-3 / 1, d64
9.1e-3 / 8.6e-3 / 1, p1100 1.00e-2 / 5.0e-3 / 0.9909 and 0.9927, b3 5.7e-3 / 3.5e-3 / 1.  At full size (cfg 2 / cfg 5, two
weight seeds) the maximum reaches 1.46e-2 and the rms 8.0e-3 — inside the bars — while the agreement of ONE run (cfg 5,
instance, seed 9) is 0.9853: like the leaky models, the 0.99 figure is not promised for every row-norm model at full size.

Shapes: p23 / d64 / p1100 of tests/test_gpu_norm_model.py (D = 128 and 64: the fused kernel unless YOLAT_RN_FUSED=0) and
b3 (n_blocks_out = 3, D = 192: the materialising route whatever the variable says).
"""
import copy
import ctypes
import functools
import hashlib
import math

import pytest
import torch

import golden_util as gu
import test_gpu_norm_model as nm

pytestmark = pytest.mark.gpu

BAR_MAX, BAR_RMS, BAR_AGREE = 1.5e-2, 1e-2, 0.99      # the standing bf16 contract
# largest max-gap measured on the MI355X over these shapes, both norms, both routes (profiles/bf16_rownorm_contract.txt)
MEASURED_MAX = 1.001e-2
NORMS = ("layer", "instance")
SHAPES = {k: nm.SHAPES[k] for k in ("p23", "d64", "p1100")}
SHAPES["b3"] = (dict(n_blocks=3, n_blocks_out=3), dict(num_proposals=40, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=60))
RN_BF16 = 0x100         # YOLAT_RN_ROUTE_BF16


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def build(yv, norm, shape, seed=31, **more):
    kw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, norm=norm)
    kw.update(SHAPES[shape][0])
    kw.update(more)
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), seed).cuda().eval()


@functools.lru_cache(maxsize=None)
def graph(shape):
    kw = SHAPES[shape][1]
    return nm._tiny_proposals(**kw) if kw["nodes_lo"] == 1 else _yv().synth_graph(n_classes=17, **kw)


@functools.lru_cache(maxsize=None)
def fp32_logits(norm, shape, edit=None):
    """the reference: the same model's fp32 forward — computed once per case, read only"""
    model = nm._edit(build(_yv(), norm, shape), edit)
    with torch.no_grad():
        return model(graph(shape), None)[0].clone()


def gap(got, want):
    got, want = got.double(), want.double()
    return (float((got - want).abs().max() / want.abs().max()), float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()),
            float((got.argmax(1) == want.argmax(1)).double().mean()))


def within_contract(name, got, want):
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
    mx, rms, agree = gap(got, want)
    print("bf16 row norm %s: max %.3e  rms %.3e  arg-max agreement %.4f (P = %d)" % (name, mx, rms, agree, got.shape[0]))
    assert mx <= BAR_MAX and rms <= BAR_RMS, "%s: max %.3e rms %.3e" % (name, mx, rms)
    if MEASURED_MAX is not None:
        assert mx <= min(BAR_MAX, 2.0 * MEASURED_MAX), "%s: max %.3e" % (name, mx)
    if got.shape[0] >= 1000:
        assert agree >= BAR_AGREE, "%s: arg-max agreement %.4f" % (name, agree)
    return mx


CASES = [(n, s, r) for n in NORMS for s in SHAPES for r in (("generic",) if s == "b3" else ("fused", "generic"))]


@pytest.mark.parametrize("norm,shape,route", CASES)
def test_bf16_forward_against_the_fp32_forward(norm, shape, route, monkeypatch):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    monkeypatch.setenv("YOLAT_RN_FUSED", "1" if route == "fused" else "0")
    want = fp32_logits(norm, shape)
    model = build(yv, norm, shape).set_eval_precision("bf16", row_norm=True)
    d = graph(shape)
    with torch.no_grad():
        got = model(d, None)[0]
        again = model(d, None)[0]
    model.check_last_status()
    within_contract("%s %s %s" % (norm, shape, route), got, want)
    assert torch.equal(got, again)                                    # two forwards: the same bits
    assert not torch.equal(got, want)                                 # the bf16 forward really ran
    plan = model._yolat_plan
    desc, h = plan._desc, plan._desc_h
    assert plan.precision == "bf16" and h is not None
    assert desc.norm == (1 if norm == "layer" else 2) and desc.act == 0
    assert desc.rn_route == RN_BF16 | (1 if route == "fused" else 2)
    assert all(bool(p) == (norm == "layer") for p in list(desc.rn_gamma) + list(desc.rn_beta))
    assert h.Wf_fold and h.tf_fold and h.Wfs_fold and h.tfs_fold and not desc.sf and not desc.Wf_hi
    assert any("rownorm" in s for s in nm._stage_names(yv, model, d))
    # the workspace tells the route: over the same descriptor with norm = batch, the bf16 hidden activations always and
    # the fp32 row range only where the pair materialises
    st = model._stage_tensors(d)
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E = ops.edge_layout(st["edge"])[0]
    need = int(lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(h), N, E, P))
    keep = desc.norm
    desc.norm = 0
    try:
        batch_like = int(lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(h), N, E, P))
    finally:
        desc.norm = keep
    hidden = 2 * P * (desc.H1 + desc.H2)
    work = 4 * int(lib.yolat_fusion_pair_eval_rn_work_elems(N, desc.F)) if route == "generic" else 0
    assert hidden + work <= need - batch_like < hidden + work + 3 * 256, (need - batch_like, hidden, work)


def test_the_norms_are_different_models_at_this_bar():
    """a bf16 forward that ran the wrong norm would not sit within the contract of the right one"""
    d = graph("p23")
    with torch.no_grad():
        got = build(_yv(), "instance", "p23").set_eval_precision("bf16", row_norm=True)(d, None)[0]
    assert gap(got, fp32_logits("layer", "p23"))[0] > 2 * BAR_MAX


@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "hipgraph"])
def test_in_place_edits_are_seen_by_the_next_forward(graphs, route, monkeypatch):
    """gamma, beta and a Linear weight edited in place are a new weight version: the centred bf16 copies are rebuilt"""
    yv = _yv()
    monkeypatch.setenv("YOLAT_RN_FUSED", "1" if route == "fused" else "0")
    model = build(yv, "layer", "p23").set_eval_precision("bf16", row_norm=True)
    dd = nm._on_device(yv, graph("p23"))
    model.use_hip_graphs(graphs)
    s = torch.cuda.Stream()
    outs = {}
    with torch.cuda.stream(s), torch.no_grad():
        outs[None] = [model(dd, None)[0].clone() for _ in range(3)]            # direct, capture, replay
        for what in ("gamma", "beta", "linear"):
            nm._edit(model, what)
            outs[what] = [model(dd, None)[0].clone() for _ in range(3)]
    torch.cuda.synchronize()
    ref = build(yv, "layer", "p23")
    for what in (None, "gamma", "beta", "linear"):
        nm._edit(ref, what)                                                    # cumulative, like the model's
        with torch.no_grad():
            want = ref(graph("p23"), None)[0]
        for o in outs[what]:
            within_contract("after editing %s" % what, o, want)
        assert torch.equal(outs[what][0], outs[what][2]), what
    assert gap(outs["gamma"][0], outs[None][0])[0] > 2 * BAR_MAX               # the edit of gamma matters at this bar


def test_prepared_graph_and_device_loader_batches_equal_the_plain_forward():
    yv = _yv()
    model = build(yv, "layer", "p23").set_eval_precision("bf16", row_norm=True)
    d = graph("p23")
    with torch.no_grad():
        want = model(d, None)[0]
        b, sl = yv.collate_to_device([d], csr=True)
        got_csr = model(b, sl)[0]
        b2, sl2 = yv.collate_to_device([d])
        got_coo = model(b2, sl2)[0]
        loader = yv.DeviceLoader([[d], [d]], slots=2)
        got_loader = [model(bb, ss)[0].clone() for bb, ss in loader]
        loader.close()
    within_contract("plain", want, fp32_logits("layer", "p23"))
    assert torch.equal(got_coo, want) and torch.equal(got_csr, want)
    assert len(got_loader) == 2 and all(torch.equal(o, want) for o in got_loader)


def _predict_model(yv, norm, classifier="softmax"):
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**dict(gu.PREDICT_OPT, norm=norm, classifier=classifier))), 5).cuda().eval()


@pytest.mark.parametrize("norm", NORMS)
def test_predict_both_ways(norm):
    from test_gpu_bf16_act_model import _predict_both
    yv = _yv()
    data, slices = yv.synth_batch(2, 21, num_proposals=300, nodes_lo=4, nodes_hi=30, edge_factor=1.3, with_roots=True)
    kw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, norm=norm)
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 3).cuda().eval()
    with torch.no_grad():                 # "has object" the arg-max of about half of the proposals: the child pass has work
        z = model(data, slices)[0]
        g = z[:, :-1].max(1).values - z[:, -1]
        model.prediction_cls[2][0].bias[model.n_classes - 1] += float(g.median())
        data._yolat_stage = None
        full32 = model(data, slices)[0].clone()
    data._yolat_stage = None
    model.set_eval_precision("bf16", row_norm=True)
    one, two = _predict_both(yv, model, data, slices)
    assert [int(v) for v in one[3]] == [int(v) for v in two[3]] and [int(v) for v in one[4]] == [int(v) for v in two[4]]
    assert len(data.roots) < len(one[3]) < data.bbox.shape[0] + 1
    assert torch.equal(one[1], two[1]) and one[0].is_cuda
    assert float((one[0] - two[0]).abs().max()) <= BAR_MAX * float(two[0].abs().max())
    within_contract("predict rows", one[0], full32[[int(v) for v in one[3]]])


@pytest.mark.parametrize("norm", NORMS)
def test_evaluate_batch_and_evaluate_submit(norm):
    from test_gpu_detect import _eval_loader
    from test_gpu_evaluate_async import _same_rep, _sync
    yv = _yv()
    model = _predict_model(yv, norm).set_eval_precision("bf16", row_norm=True)
    K = gu.PREDICT_OPT["n_classes"]
    loader = _eval_loader(yv, 4)
    for batch in loader:
        want = _sync(yv, model, copy.deepcopy(batch))
        got = yv.evaluate_batch_async(model, *copy.deepcopy(batch)).result()
        _same_rep(got, want, K)
        assert got["n_total"] > 0 and math.isfinite(got["loss"]["loss"])
    assert model._yolat_plan.precision == "bf16" and model._yolat_plan._desc.norm != 0
    data, slices = copy.deepcopy(loader[1])
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same_rep(model.evaluate_submit(data, slices).result(), want, K)
    # the loss of the bf16 evaluation against the fp32 evaluation of the same model and batch
    model32 = _predict_model(yv, norm)
    want32 = _sync(yv, model32, copy.deepcopy(loader[1]))
    assert abs(want["loss"]["loss"] - want32["loss"]["loss"]) <= 2e-2 * abs(want32["loss"]["loss"])


def _shape_of(struct):
    """a ctypes descriptor as (field, value) pairs with every pointer reduced to given / NULL, nested structures and arrays
    walked"""
    out = []
    for name, typ in struct._fields_:
        v = getattr(struct, name)
        if isinstance(v, ctypes.Structure):
            out.append((name, _shape_of(v)))
        elif isinstance(v, ctypes.Array):
            out.append((name, [_shape_of(e) if isinstance(e, ctypes.Structure) else
                               (e if isinstance(e, (int, float)) and not issubclass(typ._type_, (ctypes.c_void_p, ctypes.c_char_p))
                                else bool(e)) for e in v]))
        elif isinstance(v, (int, float)) and not issubclass(typ, ctypes.c_void_p):
            out.append((name, v))
        else:
            out.append((name, bool(v)))
    return out


def test_row_norm_has_no_effect_on_a_batch_model_and_the_plain_call_stays_loud():
    yv = _yv()
    d = graph("p23")
    a = build(yv, "batch", "p23").set_eval_precision("bf16")
    b = build(yv, "batch", "p23").set_eval_precision("bf16", row_norm=True)
    with torch.no_grad():
        assert torch.equal(a(d, None)[0], b(d, None)[0])
    assert b._yolat_plan._desc.norm == 0 and b._yolat_plan._desc.rn_route == 0
    # field for field the descriptor pair of the plain call: every number equal, every pointer given or NULL alike
    for x, y in ((a._yolat_plan._desc, b._yolat_plan._desc), (a._yolat_plan._desc_h, b._yolat_plan._desc_h)):
        assert _shape_of(x) == _shape_of(y)
    with pytest.raises(ValueError, match="norm.*row_norm"):
        build(yv, "layer", "p23").set_eval_precision("bf16")
    # the forward itself declines a row-norm base whose author did not opt in
    m = build(yv, "layer", "p23").set_eval_precision("bf16", row_norm=True)
    with torch.no_grad():
        m(d, None)
    m._yolat_plan._desc.rn_route &= ~RN_BF16
    with pytest.raises(yv._lib.YolatLibraryError, match="-2"):
        with torch.no_grad():
            m(d, None)
    m._yolat_plan._desc.rn_route |= RN_BF16


# norm = batch in bf16: (sha256 of the logits' bytes, yolat_forward_eval_bf16_workspace_bytes) per shape, taken on the parent
# commit (the commit before the bf16 row norms) with the model and graph this module builds
PARENT_BATCH_BF16 = {
    "p23": ("5e1da66313908d0d62ea208b7d82dfaf242f8dc95a3ef34ea99eab3b55d8a4c2", 564064),
    "d64": ("e9ae7633ac9e3702f87f3d34314767776968becf78b2a9b3d7078a895895c03c", 517472),
    "p1100": ("8e572563bb39c15bcc3fe5af3858900f644fb28665351abbd374f476b77c3480", 15950388),
    "b3": ("cb7ede51a8122ad1bceb3c33362dd466a0ca465805dc1728c284aa05141e2e5d", 1108900),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_bf16_forward_is_the_parents_bit_for_bit(shape):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    model = build(yv, "batch", shape).set_eval_precision("bf16")
    d = graph(shape)
    with torch.no_grad():
        got = model(d, None)[0]
    st = model._stage_tensors(d)
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E = ops.edge_layout(st["edge"])[0]
    need = int(lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(model._yolat_plan._desc_h), N, E, P))
    digest = hashlib.sha256(got.cpu().contiguous().numpy().tobytes()).hexdigest()
    print("PARENT_FIGURE %r: (%r, %d)," % (shape, digest, need))
    assert (digest, need) == PARENT_BATCH_BF16[shape]
