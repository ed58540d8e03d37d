"""GPU tests: --norm layer / instance models (torch_nn.py:23-34) on the fp32 path — eval plan, predict, training.

Bars are the project's own: logits within RTOL_FWD = 1e-4 of the largest reference logit (fp32 oracle), gradients against
the float64 oracle by the rule of test_gpu_model.py::test_other_model_shapes_match_oracle
(1e-3 * max|g_ref| + 2e-5 * gmax per tensor).

The norm sits at four sites (fusion_block, fusion_block_super, prediction_cls.0 / .1): a per-row normalisation over the
1024 / 512 / 256 columns, the same in train() and eval().  fill_state_ draws a LayerNorm's weight from (0.5, 1.5); the
instance norm has no parameters at all.  One host test (no gpu mark) pins the workspace size of a norm = batch descriptor to
the figures of the commit before the row norms existed.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import oracle_torch as orc

gpu = pytest.mark.gpu

RTOL_FWD = 1e-4
NORMS = ("layer", "instance")
SITES = ("cls_net.fusion_block", "cls_net.fusion_block_super", "prediction_cls.0", "prediction_cls.1")

# name -> (model options, synth_graph arguments).  p23: the skinny classifier route; d64 / d32: fusion_dims 64 and 32 (32: the
# generic pair route); p1100 / p2100: around YOLAT_CLS1_X6_MIN_ROWS = 1024 and YOLAT_CLS_X6_MAX_ROWS = 2048 (gemm_x6 / linear_fwd)
SHAPES = {
    "p23": (dict(), dict(num_proposals=23, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=55)),
    "d64": (dict(n_blocks_out=1), dict(num_proposals=23, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=56)),
    "d32": (dict(n_filters=32, n_blocks_out=1), dict(num_proposals=23, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=57)),
    "p1100": (dict(), dict(num_proposals=1100, nodes_lo=1, nodes_hi=3, seed=58)),
    "p2100": (dict(), dict(num_proposals=2100, nodes_lo=1, nodes_hi=3, seed=59)),
}


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _tiny_proposals(num_proposals, nodes_lo, nodes_hi, seed):
    """A graph of 1..3-node proposals built by hand (synth_graph draws src != dst inside a proposal and cannot make a
    one-node one): about 1.2 edges per node inside the proposals that have two or more nodes, none elsewhere."""
    rng = np.random.default_rng(seed)
    P = num_proposals
    n_p = rng.integers(nodes_lo, nodes_hi + 1, size=P)
    N = int(n_p.sum())
    starts = np.concatenate([[0], np.cumsum(n_p)])[:-1]
    owner = np.repeat(np.arange(P), np.where(n_p >= 2, np.ceil(1.2 * n_p).astype(np.int64), 0))
    a = rng.integers(0, 1 << 30, size=len(owner)) % n_p[owner]
    b = rng.integers(0, 1 << 30, size=len(owner)) % (n_p[owner] - 1)
    b = np.where(b >= a, b + 1, b)
    edge = np.stack([starts[owner] + a, starts[owner] + b], axis=1).astype(np.int64)
    edge = edge[rng.permutation(len(edge))]
    x = np.zeros((N, 5), dtype=np.float32)
    x[:, 3:5] = rng.random((N, 2)).astype(np.float32)
    e_attr = (rng.standard_normal((len(edge), 4)) * 0.05).astype(np.float32)
    e_attr[rng.random(len(edge)) < 0.6] = 0.0
    arrs = dict(x=x, edge=edge, e_attr=e_attr, bbox_idx=np.repeat(np.arange(P), n_p).astype(np.int64),
                labels=rng.integers(0, 17, size=P).astype(np.int64), bbox=rng.random((P, 4)).astype(np.float32),
                stat_feats=np.zeros((P, 13), np.float32))
    assert int((n_p == 1).sum()) > P // 5
    return gu.to_data(arrs, _yv().Data)


def _optkw(norm, shape, **more):
    kw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, norm=norm)
    kw.update(SHAPES[shape][0])
    kw.update(more)
    return kw


def _build(cls_mod, norm, shape, seed=31, **more):
    return gu.fill_state_(cls_mod.SparseCADGCN(cls_mod.Opt(**_optkw(norm, shape, **more))), seed)


@functools.lru_cache(maxsize=None)
def _graph(shape):
    kw = SHAPES[shape][1]
    return _tiny_proposals(**kw) if kw["nodes_lo"] == 1 else _yv().synth_graph(n_classes=17, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_eval(norm, shape, edit=None):
    """logits of the fp32 CPU oracle — computed once per case, read only.  edit: see _edit."""
    ref = _build(orc, norm, shape).eval()
    _edit(ref, edit)
    with torch.no_grad():
        return ref(_graph(shape), None)[0]


def _edit(model, what):
    """in-place edits of the weights a row-norm forward reads: a LayerNorm weight, a LayerNorm bias, a Linear weight"""
    with torch.no_grad():
        if what in ("gamma", "all"):
            model.cls_net.fusion_block[1].weight.mul_(-0.5)
            model.prediction_cls[0][1].weight[::3] = 2.0
        if what in ("beta", "all"):
            model.cls_net.fusion_block_super[1].bias.add_(0.7)
            model.prediction_cls[1][1].bias[::2] = -0.4
        if what in ("linear", "all"):
            model.cls_net.fusion_block[0].weight[::5] *= 1.5
            model.prediction_cls[0][0].weight[:, ::7] *= -1.0
    return model


def _on_device(yv, d):
    dd = yv.Data(x=d.x.cuda(), pos=d.pos)
    for k in ("edge", "e_attr", "bbox_idx", "bbox"):
        dd[k] = d[k].cuda()
    return dd


# the fusion pair of a row-norm forward: the fused kernel from YOLAT_RN_FUSED_MIN_ROWS = 12288 nodes on, the materialising route
# below — these graphs are far below, so YOLAT_RN_FUSED=1 (read by the plan when it builds its descriptor: `rn_route`) puts the
# fused kernel into the forward (d32 is off its shapes)
ROUTES = [(s, r) for s in SHAPES for r in (("generic",) if s == "d32" else ("fused", "generic"))]


@gpu
@pytest.mark.parametrize("shape,route", ROUTES)
@pytest.mark.parametrize("norm", NORMS)
def test_eval_forward_matches_oracle(norm, shape, route, monkeypatch):
    yv = _yv()
    monkeypatch.setenv("YOLAT_RN_FUSED", "1" if route == "fused" else "0")
    want = _oracle_eval(norm, shape)
    model = _build(yv, norm, shape).cuda().eval()
    d = _graph(shape)
    with torch.no_grad():
        got = model(d, None)[0]
        again = model(d, None)[0]
        sched = model.forward_scheduled(d, None)[0]
    model.check_last_status()
    desc = model._yolat_plan._desc
    assert desc.norm == (1 if norm == "layer" else 2) and desc.act == 0
    assert all(bool(p) == (norm == "layer") for p in list(desc.rn_gamma) + list(desc.rn_beta))
    assert not desc.sf and not desc.tf and not desc.sc1 and not desc.tc2          # no BatchNorm coefficients to read
    assert bool(desc.Wf_hi) == (shape != "d32")                                   # the fused kernel's shapes
    assert desc.rn_route == (1 if route == "fused" else 2)
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    stages = _stage_names(yv, model, d)
    assert any("rownorm" in s for s in stages), stages
    N, P = d.x.shape[0], d.bbox.shape[0]
    E = d.edge.shape[0]
    # the workspace tells the route: the materialising one carves its row range, the fused kernel nothing
    batch_like = _host_desc(0)
    for f in ("n_blocks", "n_blocks_out", "n_classes", "C", "F", "H1", "H2"):
        setattr(batch_like, f, getattr(desc, f))
    extra = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(desc), N, E, P)) - \
        int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(batch_like), N, E, P))
    assert (extra == 0) == (route == "fused"), (extra, route)
    scale = float(want.abs().max())
    err = float((got.cpu() - want).abs().max())
    print("eval %s %s: %.2e of %.3g" % (norm, shape, err / scale, scale))
    assert err <= RTOL_FWD * scale
    assert torch.equal(got, again)                                    # two forwards: the same bits
    assert float((sched.cpu() - want).abs().max()) <= RTOL_FWD * scale  # the Python schedule in eval mode agrees too
    if shape == "p23":
        with torch.no_grad():                                         # ... and the module-by-module path (Backbone.forward)
            modular = model.forward_modular(d, None)[0]
        assert float((modular.cpu() - want).abs().max()) <= RTOL_FWD * scale


def test_the_norm_changes_the_logits():
    """the three norms are three models: a forward that ran the wrong one would not sit within 1e-4 of the right one"""
    d = _graph("p23")
    batch = gu.fill_state_(orc.SparseCADGCN(orc.Opt(n_classes=17)), 31).eval()
    with torch.no_grad():
        outs = [batch(d, None)[0]] + [_oracle_eval(n, "p23") for n in NORMS]
    for i in range(3):
        for j in range(i):
            assert float((outs[i] - outs[j]).abs().max()) >= 0.05 * float(outs[i].abs().max())
    # the oracle's own fp32 logits are far inside the bar (float64 oracle of the same weights)
    for n in NORMS:
        r64 = _build(orc, n, "p23").double().eval()
        d64 = _data64(_yv(), d)
        with torch.no_grad():
            w64 = r64(d64, None)[0]
        assert float((_oracle_eval(n, "p23").double() - w64).abs().max()) <= 0.1 * RTOL_FWD * float(w64.abs().max())


def _stage_names(yv, model, d):
    """the stages of one profiled forward (yolat_profile_*)"""
    lib = yv._lib.lib
    lib.yolat_profile_reset()
    lib.yolat_profile_enable(1)
    try:
        with torch.no_grad():
            model(d, None)
        torch.cuda.synchronize()
    finally:
        lib.yolat_profile_enable(0)
    names = []
    for i in range(lib.yolat_profile_count()):
        buf = ctypes.create_string_buffer(160)
        ms, calls = ctypes.c_float(), ctypes.c_int()
        lib.yolat_profile_get(i, buf, 160, ctypes.byref(ms), ctypes.byref(calls), None, None)
        names.append(buf.value.decode())
    return names


# (N, E, P) -> yolat_forward_eval_workspace_bytes of the DEFAULT model's fp32 descriptor layout (n_blocks 2, n_blocks_out 2,
# C 64, F 1024, H1 512, H2 256, every bf16x6 operand present) as the commit before the row norms computed it
PARENT_WS_BYTES = {
    (165, 379, 23): 2446336,
    (10000, 40000, 400): 60905472,
    (2100, 1800, 2100): 42977024,
    (20000, 60000, 800): 88980736,
}


def _host_desc(norm_field, route=0):
    """A descriptor with the shapes and the operand PRESENCE of the default model's fp32 plan (the sizing reads nothing else)."""
    from yolat_vectorgraphicsrecognition_amd._lib import ModelEval
    d = ModelEval()
    d.n_blocks, d.n_blocks_out, d.n_classes, d.C, d.F, d.H1, d.H2 = 2, 2, 17, 64, 1024, 512, 256
    for n in ("Wf_hi", "Wf_mid", "Wf_lo", "tf_fold", "Wfs_hi", "Wfs_mid", "Wfs_lo", "tfs_fold", "Wc1_gx", "tc1_gx"):
        setattr(d, n, 1)
    d.norm = norm_field
    d.rn_route = route
    return d


@pytest.mark.host
def test_batch_descriptor_keeps_the_parents_workspace_size(monkeypatch):
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    monkeypatch.setenv("YOLAT_RN_FUSED", "1")             # the C side reads no environment: the route is the descriptor's
    for (N, E, P), want in PARENT_WS_BYTES.items():
        got = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(0)), N, E, P))
        assert got == want, (N, E, P, got)
        # a row-norm descriptor that runs the fused kernel (its shapes, N >= YOLAT_RN_FUSED_MIN_ROWS = 12288) carves nothing more ...
        rn = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(1)), N, E, P))
        assert (rn == want) == (N >= 12288), (N, rn)
        assert int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(1, route=1)), N, E, P)) == want
        assert int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(1, route=2)), N, E, P)) > want
        assert int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(0, route=2)), N, E, P)) == want
        # ... on the other route (few rows, or no split weights) exactly its row range, 256-byte aligned, nothing for a BatchNorm
        work = 4 * int(lib.yolat_fusion_pair_eval_rn_work_elems(N, 1024))
        if N < 12288:
            assert work <= rn - want < work + 512
        d0, d1 = _host_desc(0), _host_desc(2)
        d0.Wf_hi = d1.Wf_hi = None
        extra = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(d1), N, E, P)) - \
            int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(d0), N, E, P))
        assert work <= extra < work + 512 and work <= 64 << 20


@gpu
def test_batch_model_is_bit_identical_through_a_descriptor_that_leaves_norm_zero():
    """norm = batch did not move: its plan leaves `norm` and the row-norm pointers zero; two plan builds give the same bits,
    and yolat_forward_eval on that descriptor, called by hand on a fresh workspace, gives the plan's logits bit for bit (the
    golden tests of test_gpu_model.py pin the values themselves)."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(n_classes=17, norm="batch")), 31).cuda().eval()
    d = _graph("p23")
    with torch.no_grad():
        got = model(d, None)[0].clone()
    plan = model._yolat_plan
    builds = plan._desc_key
    with torch.no_grad():
        model.prediction_cls[2][0].bias.add_(0.0)                     # a weight version bump: the descriptor is rebuilt
        rebuilt = model(d, None)[0].clone()
    assert plan._desc_key == builds + 1 and torch.equal(rebuilt, got)
    desc = plan._desc
    assert desc.norm == 0 and desc.act == 0 and all(not p for p in list(desc.rn_gamma) + list(desc.rn_beta))
    st = model._stage_tensors(d)
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E, se, sc = ops.edge_layout(st["edge"])
    need = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(desc), N, E, P))
    assert need == int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(_host_desc(0)), N, E, P))
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(P, 17, device="cuda")
    check(lib.yolat_forward_eval(ctypes.byref(desc), st["x"].data_ptr(), st["x"].stride(0), st["edge"].data_ptr(), se, sc,
                                 st["e_attr"].data_ptr(), st["bbox_idx"].data_ptr(), N, E, P, out.data_ptr(), out.stride(0),
                                 ws.data_ptr(), ws.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "yolat_forward_eval")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(out, got)
    # a row norm with a leaky activation is no descriptor the forward runs
    layer = _build(yv, "layer", "p23").cuda().eval()
    with torch.no_grad():
        layer(d, None)
    bad = layer._yolat_plan._desc
    bad.act = 1
    rc = lib.yolat_forward_eval(ctypes.byref(bad), st["x"].data_ptr(), st["x"].stride(0), st["edge"].data_ptr(), se, sc,
                                st["e_attr"].data_ptr(), st["bbox_idx"].data_ptr(), N, E, P, out.data_ptr(), out.stride(0),
                                ws.data_ptr(), ws.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bad.act = 0
    assert rc == -1


@gpu
@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "hipgraph"])
def test_in_place_weight_edits_are_seen_by_the_next_forward(graphs, route, monkeypatch):
    """gamma, beta and a Linear weight edited in place, a forward (direct launches or a hipGraph replay) after each.  The
    materialising route reads W, gamma and beta by address; the fused kernel reads centred, split COPIES of the fusion
    weights, which only a rebuilt descriptor refreshes."""
    yv = _yv()
    monkeypatch.setenv("YOLAT_RN_FUSED", "1" if route == "fused" else "0")
    model = _build(yv, "layer", "p23").cuda().eval()
    dd = _on_device(yv, _graph("p23"))
    model.use_hip_graphs(graphs)
    s = torch.cuda.Stream()
    outs = {}
    with torch.cuda.stream(s), torch.no_grad():
        outs[None] = [model(dd, None)[0].clone() for _ in range(3)]            # direct, capture, replay
        for what in ("gamma", "beta", "linear"):
            _edit(model, what)
            outs[what] = [model(dd, None)[0].clone() for _ in range(3)]
    torch.cuda.synchronize()
    # the oracle with the same edits applied cumulatively
    ref = _build(orc, "layer", "p23").eval()
    d = _graph("p23")
    for what in (None, "gamma", "beta", "linear"):
        _edit(ref, what)
        with torch.no_grad():
            want = ref(d, None)[0]
        for o in outs[what]:
            assert float((o.cpu() - want).abs().max()) <= RTOL_FWD * float(want.abs().max()), what
        assert torch.equal(outs[what][0], outs[what][2]), what
    assert float((outs["linear"][0] - outs[None][0]).abs().max()) > 0.05 * float(outs[None][0].abs().max())
    assert model._yolat_plans[s.cuda_stream]._desc.rn_route == (1 if route == "fused" else 2)


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_prepared_graph_and_device_loader_batches_match_the_plain_forward(norm):
    """the other entry points of the eval plan (a batch with its prepared CSR from collate_to_device(csr=True), a
    DeviceLoader batch)"""
    yv = _yv()
    model = _build(yv, norm, "p23").cuda().eval()
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
    ref = _oracle_eval(norm, "p23")
    assert float((want.cpu() - ref).abs().max()) <= RTOL_FWD * float(ref.abs().max())
    assert torch.equal(got_coo, want)
    # (a prepared graph runs layer 0's node side as a launch of its own, on other tiles: the oracle's bar, not bits)
    assert float((got_csr.cpu() - ref).abs().max()) <= RTOL_FWD * float(ref.abs().max())
    assert len(got_loader) == 2 and all(torch.equal(o, got_csr) for o in got_loader)


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_predict_matches_the_oracle(norm):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd import architecture as A
    data, slices = gu.predict_case(yv.synth_batch)
    kw = dict(gu.PREDICT_OPT, norm=norm)
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**kw)), 40).eval()
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 40).cuda().eval()
    got = {}
    with torch.no_grad():
        want = ref.predict(data, slices)
        for one_submission in (True, False):
            A.PREDICT_ONE_SUBMISSION = one_submission
            try:
                got[one_submission] = model.predict(data, slices)
            finally:
                A.PREDICT_ONE_SUBMISSION = True
    for mode, g in got.items():
        np.testing.assert_array_equal(np.array([int(v) for v in g[3]]), np.array([int(v) for v in want[3]]))
        assert [int(v) for v in g[4]] == [int(v) for v in want[4]]
        scale = float(want[0].abs().max())
        assert float((g[0].cpu() - want[0]).abs().max()) <= RTOL_FWD * scale, mode
        np.testing.assert_allclose(g[1].cpu().numpy(), want[1].numpy(), rtol=1e-6, atol=1e-7)
    # the one-submission and the two-pass mode agree
    assert [int(v) for v in got[True][3]] == [int(v) for v in got[False][3]]
    assert float((got[True][0] - got[False][0]).abs().max()) <= RTOL_FWD * float(want[0].abs().max())


def _data64(yv, d):
    d64 = yv.Data(x=d.x.double(), pos=d.pos)
    for k in ("edge", "bbox_idx", "bbox", "labels", "stat_feats"):
        d64[k] = d[k]
    d64.e_attr = d.e_attr.double()
    return d64


def _train_once(yv, norm, dropout, seed=None):
    kw = _optkw(norm, "p23", dropout=dropout)
    model = _build(yv, norm, "p23", dropout=dropout).cuda().train()
    d = _graph("p23")
    if seed is not None:
        torch.manual_seed(seed)
    out = model(d, None)
    loss = yv.DetectionLoss(yv.Opt(**kw))(out, d)["loss"]
    loss.backward()
    return model, out[0].detach(), loss.detach()


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_training_step_matches_the_float64_oracle(norm):
    yv = _yv()
    d = _graph("p23")
    model, logits, loss = _train_once(yv, norm, 0.0)
    ref64 = _build(orc, norm, "p23").double().train()
    d64 = _data64(yv, d)
    rout = ref64(d64, None)
    rloss = orc.DetectionLoss(orc.Opt(**_optkw(norm, "p23")))(rout, d64)["loss"]
    rloss.backward()
    assert float((logits.cpu().double() - rout[0].detach()).abs().max()) <= RTOL_FWD * float(rout[0].detach().abs().max())
    assert abs(float(loss) - float(rloss)) <= RTOL_FWD * abs(float(rloss))
    gmax = max(float(p.grad.abs().max()) for p in ref64.parameters())
    names = [n for n, _ in model.named_parameters()]
    assert names == [n for n, _ in ref64.named_parameters()]
    # index 1 of the four sites: a LayerNorm's weight and bias get gradients, an instance norm has no entries there
    at1 = [n for n in names if any(n.startswith(s + ".1.") for s in SITES)]
    assert len(at1) == (8 if norm == "layer" else 0)
    for (n, p), (_, q) in zip(model.named_parameters(), ref64.named_parameters()):
        assert p.grad is not None, n
        err = float((p.grad.cpu().double() - q.grad).abs().max())
        if n in at1:
            print("%s: %.2e of %.3g" % (n, err, float(q.grad.abs().max())))
        assert err <= 1e-3 * max(float(q.grad.abs().max()), 1e-12) + 2e-5 * gmax, (n, err)
    # the same state twice: the same bits
    model2, logits2, loss2 = _train_once(yv, norm, 0.0)
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2)
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    # train() and eval() are the same arithmetic at the four sites, but not in the conv layers' BatchNorms: the running
    # statistics moved, nothing at the four sites has any
    assert not any("running" in k for k in model.state_dict() if any(k.startswith(s) for s in SITES))


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_trainer_step_matches_the_oracle_step(norm):
    """One Trainer.step (it falls back to the Python schedule by itself: the one-call plan declines a row-norm model) against
    orc.train_step in float64 with torch.optim.Adam(lr, weight_decay).  Parameters are compared where the first Adam step is
    well conditioned (the rule of test_gpu_model.py::_check_param_after: |g| above 50x the gradient tolerance), to fp32
    rounding of the parameter (2e-6 relative + 2e-7)."""
    yv = _yv()
    d = _graph("p23")
    kw = _optkw(norm, "p23")
    model = _build(yv, norm, "p23").cuda()
    tr = yv.Trainer(model, yv.Opt(**kw), lr=2.5e-4, weight_decay=1e-5)
    assert tr.plan.model_fits() is False
    for p in model.parameters():
        assert p.data_ptr() % 16 == 0
    loss = tr.step(d)
    assert tr.plan_steps == 0
    ref64 = _build(orc, norm, "p23").double().train()
    optim = torch.optim.Adam(ref64.parameters(), lr=2.5e-4, weight_decay=1e-5)
    d64 = _data64(yv, d)
    rloss, _ = orc.train_step(ref64, orc.DetectionLoss(orc.Opt(**kw)), optim, d64)
    gmax = max(float(p.grad.abs().max()) for p in ref64.parameters())
    checked = 0
    for (n, p), (_, q) in zip(model.named_parameters(), ref64.named_parameters()):
        g = q.grad
        mask = g.abs() > max(50 * 1e-3 * float(g.abs().max()), 20 * 2e-5 * gmax)
        got, want = p.detach().cpu().double()[mask], q.detach()[mask]
        checked += int(mask.sum())
        assert bool(((got - want).abs() <= 2e-6 * want.abs() + 2e-7).all()), n
    assert checked > 1000
    assert torch.isfinite(loss)
    assert abs(float(loss) - float(rloss)) <= RTOL_FWD * abs(float(rloss))
    # a second step runs (Adam state); a LayerNorm's weight and bias move like any parameter
    if norm == "layer":
        before = model.cls_net.fusion_block[1].weight.detach().clone()
    tr.step(d)
    if norm == "layer":
        assert not torch.equal(model.cls_net.fusion_block[1].weight.detach(), before)


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_training_with_dropout_runs(norm):
    """Dropout2d(0.3) behind prediction_cls.1 masks the materialised row-norm output: shapes, finiteness, a gradient for
    every parameter, and the same seed giving the same step (the mask follows torch.manual_seed)."""
    yv = _yv()
    model, logits, loss = _train_once(yv, norm, 0.3, seed=5)
    assert logits.shape == (23, 17) and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
    model2, logits2, loss2 = _train_once(yv, norm, 0.3, seed=5)
    assert torch.equal(logits, logits2)
    model3, logits3, _ = _train_once(yv, norm, 0.3, seed=6)
    assert not torch.equal(logits, logits3)


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_standalone_mlp_forward_and_backward_match_the_oracle(norm):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd.nn_modules import MLP
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 70, generator=g)
    w = torch.randn(37, 40, generator=g)
    mlp = gu.fill_state_(MLP([70, 96, 40], "relu", norm), 9)
    ref = gu.fill_state_(orc.MLP([70, 96, 40], "relu", norm), 9).double()
    assert list(mlp.state_dict()) == list(ref.state_dict())
    mlp = mlp.cuda().train()
    ref.train()
    xg = x.cuda().requires_grad_(True)
    y = mlp(xg)
    (y * w.cuda()).sum().backward()
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    (yr * w.double()).sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) <= RTOL_FWD * float(yr.abs().max())
    gmax = max(float(p.grad.abs().max()) for p in ref.parameters())
    pairs = list(zip(mlp.named_parameters(), ref.parameters())) + [(("x", xg), xr)]
    for (n, p), q in pairs:
        err = float((p.grad.cpu().double() - q.grad).abs().max())
        assert err <= 1e-3 * max(float(q.grad.abs().max()), 1e-12) + 2e-5 * gmax, (n, err)
    mlp.eval(); ref.eval()
    with torch.no_grad():
        ye, yre = mlp(x.cuda()), ref(x.double())
    assert float((ye.cpu().double() - yre).abs().max()) <= RTOL_FWD * float(yre.abs().max())
    assert torch.equal(ye, y.detach())                       # train() and eval(): one arithmetic


def _eval_loader(yv, seed):
    """Two batches of two synthetic items each, with the fields the reference's evaluation loop reads (the builder of
    test_gpu_detect.py, copied)."""
    rng = np.random.default_rng(seed)
    batches = []
    for b in range(2):
        items = []
        for i in range(2):
            kw = dict(gu.PREDICT_CASE)
            kw.pop("n_graphs", None)
            kw.pop("seed", None)
            it = yv.synth_graph(seed=seed * 100 + b * 10 + i, **kw)
            P = it.bbox.shape[0]
            k = min(6, P)
            pick = rng.choice(P, size=k, replace=False)
            it.gt_bbox = it.bbox[pick].clone()
            it.gt_labels = torch.from_numpy(rng.integers(0, gu.PREDICT_OPT["n_classes"] - 1, size=k)).long()
            it.has_obj = torch.ones(P, dtype=torch.long)
            it.width = torch.tensor([1000.0])
            it.height = torch.tensor([800.0])
            items.append(it)
        batches.append(yv.collate(items))
    return batches


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_detect_batch_is_predict_plus_scores_plus_batched_nms(norm):
    """detect_batch rides the eval plan: its detections are those of predict (checked against the oracle's logits here) +
    detect_scores + the batched NMS."""
    import copy
    yv = _yv()
    kw = dict(gu.PREDICT_OPT, norm=norm)
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 5).cuda().eval()
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**kw)), 5).eval()
    batch = _eval_loader(yv, 6)[1]
    got = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    data, slices = copy.deepcopy(batch)
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    data_ref = copy.deepcopy(data)                     # (predict caches device state on the batch it is given)
    with torch.no_grad():
        out = model.predict(data, slices)
        want_out = ref.predict(data_ref, slices)
    assert [int(v) for v in out[3]] == [int(v) for v in want_out[3]]
    assert float((out[0].cpu() - want_out[0]).abs().max()) <= RTOL_FWD * float(want_out[0].abs().max())
    ptr = [int(v) for v in out[4]]
    scale = torch.tensor([[1000.0, 800.0, 1000.0, 800.0]] * 2).cuda()
    pred = yv.ops.detect_scores(out[0].float(), out[1].float().contiguous(),
                                torch.tensor(ptr, dtype=torch.int32, device="cuda"), scale)
    want = yv.non_max_suppression_batched(pred, ptr, conf_thres=0.05, iou_thres=0.5)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.is_cuda and g.shape[0] > 0 and torch.equal(g, w)


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_evaluation_loop_runs_a_row_norm_model(norm):
    """evaluation.test (yv.evaluate) over two batches rides the eval plan: a finite report of ten mAPs, the default and the
    device post-processing agree, and a second run gives the same number (the forward's values are checked against the
    oracle by the tests above)."""
    import copy
    yv = _yv()
    kw = dict(gu.PREDICT_OPT, norm=norm)
    opt = yv.Opt(**kw)
    model = gu.fill_state_(yv.SparseCADGCN(opt), 5).cuda()
    loader = _eval_loader(yv, 3)
    want = yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt), opt)
    ref = opt.test_report
    opt_d = yv.Opt(**kw)
    opt_d.device_postprocess = True
    got = yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt_d), opt_d)
    rep = opt_d.test_report
    assert got is not None and len(rep["map"]) == 10 and all(np.isfinite(float(v)) for v in rep["map"]) and all(np.isfinite(v) for v in rep["loss"].values())
    assert rep["top1"] == ref["top1"] and rep["loss"] == ref["loss"]
    np.testing.assert_allclose(rep["map"], ref["map"], rtol=0, atol=1e-6)
    assert abs(got - want) <= 1e-6
    opt_e = yv.Opt(**kw)
    opt_e.device_postprocess = True
    assert yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt_e), opt_e) == got      # deterministic
