"""GPU tests (-m gpu) of the bf16-storage eval forward (csrc/bf16_eval.hip, yolat_forward_eval_bf16): the precision
mode of BASELINE.json configs[4] ("N=200k / E=1.2M, n_blocks=4, bf16").  SURVEY.md §8c: "bf16 variant compared to the
fp32 oracle at <= 1e-2 rel with fp32 accumulation" — here 1e-2 of the logits' scale, against the golden vectors of
the reference's own modules, the CPU oracle, and the fp32 HIP path at full size."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import oracle_torch as orc

pytestmark = pytest.mark.gpu

# What bf16 STORAGE can deliver: every stored activation / weight is rounded to 8 mantissa bits (relative error up
# to 2^-9, rms 2^-9/sqrt(3) = 1.1e-3) and a 4-block forward has ~27 such roundings between x and the logits (per
# layer: layer output, [W1a-W1b | W1b], U|V, hidden activation, W2; then Wf, the pooled matrix, the classifier
# weights/activations) -> expected rms error sqrt(27) * 1.1e-3 = 5.7e-3 of the logits' rms.  Measured
# (tools/exp/bf16_err.py, 2000 proposals): rms 4.0e-3 (2 blocks) .. 6.4e-3 (4 blocks), max 0.65e-2 .. 1.2e-2 of
# the scale, arg-max agreement >= 98 %.  SURVEY.md 8c's "<= 1e-2 rel" is asserted on the rms; the element-wise
# maximum (a 4-5 sigma event over 10^4..10^6 logits) gets 2e-2.
RTOL_BF16 = 2e-2        # max |logit error| / max |logit|
RMS_BF16 = 1e-2         # rms error / rms logit


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _model(yv, optkw, seed):
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), seed).cuda().eval()


def _check(name, got, want, depth_factor=1.0):
    """depth_factor: the error budget grows with the number of rounding stages (~5 per conv layer); the stated
    bounds are for the reference's depths (n_blocks <= 4), deeper stacks get a proportionally wider band."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    rms = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    assert err <= RTOL_BF16 * depth_factor * scale, "%s: max err %.3e of scale %.3e (rel %.2e)" % (name, err, scale,
                                                                                                    err / scale)
    assert rms <= RMS_BF16 * depth_factor, "%s: rms rel err %.2e" % (name, rms)
    return err / scale


def test_f32_to_bf16_is_round_to_nearest_even():
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(100001, generator=g) * 3.0, torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, 1e-30, 3.3895e38]),
                   # exact ties: mantissa bits below bf16 precision = 0x8000 with even / odd kept bit
                   torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0x3F80FFFF], dtype=torch.int64).to(torch.int32)
                   .view(torch.float32)]).cuda()
    out = torch.empty(x.numel() + (x.numel() & 1), dtype=torch.bfloat16, device="cuda")
    check(lib.yolat_f32_to_bf16(x.data_ptr(), x.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "yolat_f32_to_bf16")
    want = x.to(torch.bfloat16)
    assert torch.equal(out[:x.numel()].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("kind", ["small", "medium", "deep"])
def test_bf16_eval_forward_vs_reference_golden(kind, golden_dir):
    yv = _yv()
    z = np.load(os.path.join(golden_dir, "model_%s.npz" % kind))
    arrs, optkw = gu.graph_case(kind)
    model = _model(yv, optkw, int(z["seed"])).set_eval_precision("bf16")
    with torch.no_grad():
        pred, bbox = model(gu.to_data(arrs, yv.Data), None)
    model._yolat_plan.check_status()
    assert model._yolat_plan.precision == "bf16"
    ref = gu.unpack("eval_logits", z)
    got = pred.detach().cpu().double().numpy().reshape(-1)
    want = ref["full"].astype(np.float64) if "full" in ref else None
    if want is None:
        got, want = got[::int(ref["stride"])], ref["sample"].astype(np.float64)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= RTOL_BF16 * scale
    assert np.sqrt(np.mean((got - want) ** 2) / np.mean(want ** 2)) <= RMS_BF16
    np.testing.assert_array_equal(bbox.cpu().numpy(), arrs["bbox"])


@pytest.mark.parametrize("cin,blocks,blocks_out,classes,seed", [(5, 2, 2, 17, 1), (6, 3, 2, 22, 2), (5, 4, 2, 17, 3),
                                                                 (3, 2, 1, 5, 4), (5, 4, 4, 17, 5), (5, 6, 5, 17, 6),
                                                                 (5, 3, 3, 17, 7)])
def test_bf16_eval_forward_vs_cpu_oracle(cin, blocks, blocks_out, classes, seed):
    """model shapes incl. the YOLaT++ depth (n_blocks=4, n_blocks_out=2), the 192-wide (n_blocks_out=3: the rows kernel's
    zero-filled LDS columns), the 256-wide (n_blocks_out=4) and the
    > 256-wide (n_blocks_out=5: per-tile fallback of the fusion GEMM) concatenations, on a ragged graph (proposals of 2..40 nodes,
    nodes without in-edges, duplicate edges) against the CPU oracle in fp32."""
    yv = _yv()
    optkw = dict(n_classes=classes, n_blocks=blocks, n_blocks_out=blocks_out, in_channels=cin)
    d = yv.synth_graph(num_proposals=211, nodes_lo=2, nodes_hi=40, edge_factor=2.1, n_classes=classes, seed=70 + seed)
    if cin != 5:
        d.x = torch.randn(d.x.shape[0], cin, generator=torch.Generator().manual_seed(cin)) * 0.7
    d.edge = torch.cat([d.edge, d.edge[:17]], 0)            # duplicate edges are defined by the PyG semantics
    d.e_attr = torch.cat([d.e_attr, d.e_attr[:17]], 0)
    model = _model(yv, optkw, 40 + seed).set_eval_precision("bf16")
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**optkw)), 40 + seed).eval()
    with torch.no_grad():
        got = model(d, None)[0]
        want = ref(d, None)[0]
    model._yolat_plan.check_status()
    _check("logits", got, want, depth_factor=max(1.0, blocks / 4.0))
    # the same model object switches back to the fp32 plan (1e-4 bar) on request
    model.set_eval_precision("fp32")
    with torch.no_grad():
        got32 = model(d, None)[0].cpu()
    assert model._yolat_plan.precision == "fp32"
    assert float((got32 - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_bf16_edge_cases_no_edges_and_single_node_proposals():
    yv = _yv()
    optkw = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
    model = _model(yv, optkw, 3).set_eval_precision("bf16")
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**optkw)), 3).eval()
    d = yv.synth_graph(num_proposals=7, nodes_lo=3, nodes_hi=6, seed=11)
    d.edge = torch.zeros((0, 2), dtype=torch.long)
    d.e_attr = torch.zeros((0, 4))
    with torch.no_grad():
        _check("E=0", model(d, None)[0], ref(d, None)[0])
    model._yolat_plan.check_status()
    # P > 65535 one-to-three-node proposals (grid.y chunking of the pooling prologue), star edges
    big = yv.synth_graph(num_proposals=70000, nodes_lo=1, nodes_hi=3, edge_factor=0.0, seed=12, edges_per_proposal=0)
    N = big.x.shape[0]
    owner = big.bbox_idx.numpy()
    first = np.searchsorted(owner, owner)
    src = np.arange(N)
    has_pair = first != src
    e = np.stack([src[has_pair], first[has_pair]], 1)
    big.edge = torch.from_numpy(e.astype(np.int64))
    big.e_attr = torch.from_numpy((np.random.default_rng(0).standard_normal((len(e), 4)) * 0.05).astype(np.float32))
    with torch.no_grad():
        got = model(big, None)[0]
        want = ref(big, None)[0]
    assert got.shape == (70000, 17)
    _check("P=70000", got, want)
    model._yolat_plan.check_status()


def test_bf16_full_size_cfg2_vs_oracle_and_determinism():
    yv = _yv()
    data, slices, optkw, _ = yv.config("2")
    model = _model(yv, optkw, 7).set_eval_precision("bf16")
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**optkw)), 7).eval()
    with torch.no_grad():
        got = model(data, slices)[0].clone()
        again = model(data, slices)[0]
        want = ref(data, slices)[0]
    assert torch.equal(got, again)                      # integer-atomic max + fixed summation orders
    _check("cfg2", got, want)


def test_bf16_full_size_cfg5_vs_fp32_path_and_size_independent_properties():
    """configs[4] (N=200k / E=1.2M / P=8000, n_blocks=4) — too big for the CPU oracle: the bf16 forward is compared
    with the fp32 HIP forward (itself pinned to 1e-4 by the other tests) and must be deterministic and
    block-diagonal (the forward of the two proposal halves stacked equals the forward of the whole graph)."""
    yv = _yv()
    data, slices, optkw, _ = yv.config("5")
    model = _model(yv, optkw, 9)
    with torch.no_grad():
        want = model(data, slices)[0].clone()
        model.set_eval_precision("bf16")
        got = model(data, slices)[0].clone()
        again = model(data, slices)[0]
    model._yolat_plan.check_status()
    assert torch.equal(got, again)
    _check("cfg5 bf16 vs fp32", got, want)
    N, P = data.x.shape[0], data.bbox.shape[0]
    bb = data.bbox_idx.numpy()
    node_ptr = np.searchsorted(bb, np.arange(P + 1))
    owner_e = bb[data.edge[:, 0].numpy()]

    def sub(p_lo, p_hi):
        n_lo, n_hi = node_ptr[p_lo], node_ptr[p_hi]
        em = (owner_e >= p_lo) & (owner_e < p_hi)
        d = yv.Data(x=data.x[n_lo:n_hi], pos=data.pos[n_lo:n_hi])
        d.edge = data.edge[em] - int(n_lo)
        d.e_attr = data.e_attr[em]
        d.bbox_idx = data.bbox_idx[n_lo:n_hi] - p_lo
        d.bbox = data.bbox[p_lo:p_hi]
        d.stat_feats = data.stat_feats[p_lo:p_hi]
        return d

    with torch.no_grad():
        a = model(sub(0, P // 2), None)[0]
        b = model(sub(P // 2, P), None)[0]
    # every row's arithmetic is identical in the split run (per-row GEMMs, per-node sums in CSR order)
    assert torch.equal(torch.cat([a, b], 0), got)


def test_bf16_unsupported_shapes_fail_loudly():
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import YolatLibraryError
    optkw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, n_filters=32)
    model = yv.SparseCADGCN(yv.Opt(**optkw)).cuda().eval().set_eval_precision("bf16")
    d = yv.synth_graph(num_proposals=5, nodes_lo=3, nodes_hi=6, seed=1)
    with pytest.raises((YolatLibraryError, ValueError)), torch.no_grad():
        model(d, None)
    with pytest.raises(ValueError):
        model.set_eval_precision("fp16")


def test_bf16_hip_graph_replay_and_concurrent_streams_match_direct_launches():
    """the bf16 plan under the two serving-side mechanisms of the fp32 plan: hipGraph replay (same input buffers) and
    independent forwards on concurrent streams — both bit-identical to a direct launch on the default stream."""
    yv = _yv()
    optkw = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
    model = _model(yv, optkw, 21).set_eval_precision("bf16")
    d = yv.synth_graph(num_proposals=150, nodes_lo=5, nodes_hi=30, edge_factor=2.5, seed=5)
    for k in ("x", "edge", "e_attr", "bbox_idx", "bbox"):
        d[k] = d[k].cuda()
    with torch.no_grad():
        want = model(d, None)[0].clone()
        model.use_hip_graphs(True)
        outs = [model(d, None)[0].clone() for _ in range(4)]       # launch, capture, replay, replay
        model.use_hip_graphs(False)
    for o in outs:
        assert torch.equal(o, want)
    streams = [torch.cuda.Stream() for _ in range(4)]
    res = []
    with torch.no_grad():
        for rep in range(3):
            for s in streams:
                with torch.cuda.stream(s):
                    res.append(model(d, None)[0])
    torch.cuda.synchronize()
    for o in res:
        assert torch.equal(o, want)


# ---------------------------------------------------------------------------------------------
# bf16-storage TRAINING step (BASELINE.json configs[4]; SURVEY.md section 8 row g)
# ---------------------------------------------------------------------------------------------
def _train_once(yv, optkw, data, seed, precision, slices=None):
    opt = yv.Opt(**optkw)
    model = gu.fill_state_(yv.SparseCADGCN(opt), seed).cuda()
    tr = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5, precision=precision)
    if hasattr(data, "_yolat_stage"):
        data._yolat_stage = None
    loss = tr.step(data, slices)
    grads = {n: tr.flat.grad_views[id(p)].detach().clone() for n, p in model.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in model.named_buffers() if b.is_floating_point()}
    return float(loss), grads, bufs


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _perturbed_fp32(yv, optkw, data, seed, slices=None):
    """Sensitivity baseline: the fp32 step on node features carrying bf16-sized relative noise (uniform in
    +-2^-9).  A freshly initialised YOLaT network is discontinuous in its activations (per-proposal max pooling picks
    rows, ReLUs gate), so ANY 0.2 % perturbation moves the gradients by ~10 %; the bf16-storage step is held to the
    same scale, not to the rounding unit."""
    x0 = data.x
    g = torch.Generator().manual_seed(1)
    data.x = x0 * (1 + (torch.rand(x0.shape, generator=g) - 0.5) * 2 ** -8)
    try:
        return _train_once(yv, optkw, data, seed, "fp32", slices)
    finally:
        data.x = x0


def _cos(ga, gb):
    a = torch.cat([ga[n].flatten().double() for n in ga])
    b = torch.cat([gb[n].flatten().double() for n in ga])
    return float(a @ b / (a.norm() * b.norm()))


def _check_bf16_step(yv, optkw, data, seed, slices=None, loss_tol=1e-3):
    l32, g32, b32 = _train_once(yv, optkw, data, seed, "fp32", slices)
    l16, g16, b16 = _train_once(yv, optkw, data, seed, "bf16", slices)
    lp, gp, _ = _perturbed_fp32(yv, optkw, data, seed, slices)
    assert np.isfinite(l16) and abs(l16 - l32) <= loss_tol * abs(l32), (l16, l32)
    assert any(not torch.equal(g16[n], g32[n]) for n in g32)          # the bf16 path really ran
    cos16, cosp = _cos(g32, g16), _cos(g32, gp)
    assert cos16 >= 0.99 and (1 - cos16) <= 2.5 * (1 - cosp) + 1e-4, (cos16, cosp)
    gscale = max(_rms(v) for v in g32.values())
    for n in g32:
        assert bool(torch.isfinite(g16[n]).all()), n
        err16, errp = _rms(g16[n] - g32[n]), _rms(gp[n] - g32[n])
        # per tensor: within 2.5x of what the bf16-sized input perturbation does to the fp32 step, + a floor for the
        # mathematically-zero gradients (biases in front of a BatchNorm): there the sum over E rounded rows is a random
        # walk of rounding errors, sqrt(E) * 2^-9 * rms — a few percent of the largest gradient at E = 1.2 M
        assert err16 <= 2.5 * errp + 2e-2 * _rms(g32[n]) + 4e-2 * gscale, \
            "%s: rms err %.3e (perturbed fp32: %.3e) vs rms %.3e" % (n, err16, errp, _rms(g32[n]))
    for n in b32:
        assert float((b16[n] - b32[n]).abs().max()) <= 1e-2 * float(b32[n].abs().max()) + 1e-6, n
    return l16, g16, cos16, cosp


def _perturb_x(data, seed=1):
    """data.x with bf16-sized relative noise (uniform in +-2^-9), as _perturbed_fp32 applies it."""
    g = torch.Generator().manual_seed(seed)
    return data.x * (1 + (torch.rand(data.x.shape, generator=g) - 0.5) * 2 ** -8)


def bf16_grads_vs_fp64_oracle(g16, g64, g64p, name):
    """Every gradient tensor of the bf16-STORAGE step against the float64 CPU ORACLE (not against the HIP fp32 step), at
    the tensor's own scale:   rms(g16_n - g64_n) <= 4 * rms(g64p_n - g64_n) + 2e-2 * rms(g64_n)
    g64p = the same float64 oracle on node features carrying bf16-sized noise: the oracle's own statement of what ONE
    2^-9 relative perturbation of stored values is worth for that tensor (the network is discontinuous: per-proposal
    arg-max, ReLU gates); the bf16 step rounds at every stored [E,64] activation and gradient of every layer, hence the
    factor 4 (measured, tools/exp/bf16_grad_bound_which_tensor.py on the 4-block fixture: the tensor that needs more than
    2.5 is `prediction_cls.1.1.bias` — the BatchNorm shift of the classifier's second block — at 3.0; next
    `prediction_cls.1.0.weight` 2.5, `prediction_cls.0.1.weight` 2.3, every conv-layer tensor <= 1.4: the classifier sits
    behind the per-proposal arg-max of ALL layers, so its gradients collect every layer's rounding while the probe perturbs
    the input once).  2e-2 = the bf16 term: ~5 stored roundings of 2^-9 between a gradient and its tensor.
    The one exception, as in tests/test_gpu_configs.py::_grad_check_per_tensor: a MATHEMATICALLY ZERO gradient (the bias
    of a Linear in front of a BatchNorm, |g64| < 1e-9 gmax) is a random walk of rounding errors over E rows,
    sqrt(E) * 2^-9 * rms(dY) — bounded by 4e-2 of the largest tensor rms."""
    gmax = max(float(v.abs().max()) for v in g64.values())
    gscale = max(_rms(v) for v in g64.values())
    bad = []
    for n, ref in g64.items():
        a = g16[n].detach().cpu().double()
        assert bool(torch.isfinite(a).all()), n
        err, sens, rms = _rms(a - ref), _rms(g64p[n] - ref), _rms(ref)
        tol = 4.0 * sens + 2e-2 * rms
        if float(ref.abs().max()) < 1e-9 * gmax:
            tol = 4e-2 * gscale
        if err > tol:
            bad.append("%s err %.3e tol %.3e (sens %.3e rms %.3e)" % (n, err, tol, sens, rms))
    assert not bad, "%s: %s" % (name, "; ".join(bad[:8]))


def test_bf16_storage_train_step_gradients_match_fp64_oracle_deep_fixture():
    """The 4-block golden fixture ("deep", K = 22): loss and EVERY gradient tensor of the bf16-storage training step
    against the float64 CPU oracle (cad_recognition/train.py:263-284), not against the HIP fp32 step."""
    yv = _yv()
    arrs, optkw = gu.graph_case("deep")
    data = gu.to_data(arrs, yv.Data)

    def oracle(x):
        ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**optkw)), 77).double().train()
        d = gu.to_data(arrs, yv.Data)
        d.x = x.double(); d.e_attr = d.e_attr.double()
        out = ref(d, None)
        loss = orc.DetectionLoss(orc.Opt(**optkw))(out, d)["loss"]
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().double() for n, p in ref.named_parameters()}

    l64, g64 = oracle(data.x)
    _, g64p = oracle(_perturb_x(data))
    l16, g16, _ = _train_once(yv, optkw, data, 77, "bf16")
    assert abs(l16 - l64) <= 5e-3 * abs(l64), (l16, l64)
    bf16_grads_vs_fp64_oracle(g16, g64, g64p, "deep fixture, bf16 storage")


@pytest.mark.parametrize("kind", ["medium", "deep"])
def test_bf16_storage_train_step_matches_fp32_step(kind):
    """The [E,64] activations of the edge MLP and their gradients stored as bfloat16 (fp32 accumulation, statistics,
    parameters): loss within 1e-3 (2 blocks) / 5e-3 (4-block fixture) of the fp32 HIP step; gradients as close to it as the fp32 step itself is under a
    bf16-sized perturbation of its input (see _perturbed_fp32); BatchNorm running statistics within 1e-2; deterministic."""
    yv = _yv()
    arrs, optkw = gu.graph_case(kind)
    data = gu.to_data(arrs, yv.Data)
    assert arrs["edge"].shape[0] >= 2 * arrs["x"].shape[0]          # the factorised / bf16 path applies
    # loss: <= 1e-3 for the 2-block case; the 4-block fixture (few hundred rows per BatchNorm) moves by 2e-3
    l16, g16, _, _ = _check_bf16_step(yv, optkw, data, 3, loss_tol=1e-3 if kind == "medium" else 5e-3)
    l16b, g16b, _ = _train_once(yv, optkw, data, 3, "bf16")
    assert l16b == l16 and all(torch.equal(g16[n], g16b[n]) for n in g16)


def test_bf16_storage_train_step_cfg5():
    """configs[4] at full size (N = 200k, E = 1.2M, n_blocks = 4): the bf16-storage step against the fp32 step."""
    yv = _yv()
    data, slices, optkw, _ = yv.config("5")
    l16, _, cos16, cosp = _check_bf16_step(yv, optkw, data, 5, slices, loss_tol=2e-3)
    print("cfg 5 bf16-storage step: loss %.6f, gradient cosine vs fp32 %.5f (fp32 under 2^-9 input noise: %.5f)" %
          (l16, cos16, cosp))


def test_bf16_storage_ops_match_fp32_ops_on_the_same_values():
    """Every bf16-storage op against its fp32 twin fed the widened bf16 values: the arithmetic is the same, only the
    final store rounds (bf16 MFMA GEMMs: products exact, fp32 accumulation in a different order)."""
    yv = _yv()
    N, E = 500, 6000
    rng = np.random.default_rng(3)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    g = yv.ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).cuda(),
                           torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32)).cuda(), None, N, 1)
    tg = torch.Generator().manual_seed(0)
    bf = torch.bfloat16
    H = torch.randn(E, 64, generator=tg).cuda().to(bf)
    G = torch.randn(E, 64, generator=tg).cuda().to(bf)
    W = (torch.randn(64, 64, generator=tg) / 8).cuda()
    b = torch.randn(64, generator=tg).cuda() * 0.1
    sc, sh = (torch.rand(64, generator=tg) + 0.5).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda()
    # Linear + statistics
    Y16, Y32 = torch.empty(E, 64, device="cuda", dtype=bf), torch.empty(E, 64, device="cuda")
    st16, st32 = yv.ops.stats_buffer(E, 64, "cuda"), yv.ops.stats_buffer(E, 64, "cuda")
    yv.ops.linear_fwd(H, W, b, Y16, a_pro=(sc, sh), a_relu=True, stats=st16)
    A32 = torch.relu(H.float() * sc + sh).to(bf).float()              # the prologue result is re-rounded to bf16
    yv.ops.linear_fwd(A32, W.to(bf).float(), b, Y32, stats=st32)
    assert float((Y16.float() - Y32).abs().max()) <= 2 ** -7 * float(Y32.abs().max())
    # (sum, M2) per 32-row group: the kernel's prologue is an fma, torch's a mul + add, so now and then one element
    # rounds to the neighbouring bf16 value
    nst = 2 * ((E + 31) // 32) * 64                                   # the written part of the (padded) buffer
    assert float((st16[:nst] - st32[:nst]).abs().max()) <= 2e-2 * float(st32[:nst].abs().max())
    # dX = dY . W
    X16, X32 = torch.empty(E, 64, device="cuda", dtype=bf), torch.empty(E, 64, device="cuda")
    yv.ops.linear_fwd_wt(G, W, X16)
    yv.ops.linear_fwd_wt(G.float(), W.to(bf).float(), X32)
    assert float((X16.float() - X32).abs().max()) <= 2 ** -7 * float(X32.abs().max())
    # dW = dY^T . pro(A)  (fp32 accumulation of exact widened values: agrees to fp32 round-off)
    dW16, db16, dW32, db32 = (torch.empty(64, 64, device="cuda"), torch.empty(64, device="cuda"),
                              torch.empty(64, 64, device="cuda"), torch.empty(64, device="cuda"))
    yv.ops.linear_bwd_w(G, H, dW16, db16, a_pro=(sc, sh), a_relu=True)
    yv.ops.linear_bwd_w(G.float(), H.float(), dW32, db32, a_pro=(sc, sh), a_relu=True)
    assert float((dW16 - dW32).abs().max()) <= 1e-5 * float(dW32.abs().max())
    assert float((db16 - db32).abs().max()) <= 1e-5 * float(db32.abs().max())
    # BatchNorm + ReLU backward
    mean, invstd = H.float().mean(0), 1.0 / (H.float().var(0, unbiased=False) + 1e-5).sqrt()
    dg16, dbt16, dg32, dbt32 = [torch.empty(64, device="cuda") for _ in range(4)]
    D16, D32 = torch.empty(E, 64, device="cuda", dtype=bf), torch.empty(E, 64, device="cuda")
    yv.ops.bn_relu_bwd(G, H, sc, mean, invstd, sc, sh, True, dg16, dbt16, D16)
    yv.ops.bn_relu_bwd(G.float(), H.float(), sc, mean, invstd, sc, sh, True, dg32, dbt32, D32)
    assert float((dg16 - dg32).abs().max()) <= 1e-4 * float(dg32.abs().max())
    assert float((dbt16 - dbt32).abs().max()) <= 1e-4 * float(dbt32.abs().max())
    assert torch.equal(D16, D32.to(bf)) or float((D16.float() - D32).abs().max()) <= 2 ** -7 * float(D32.abs().max())
    # per-node sums for the factorised backward
    x = torch.randn(N, 64, generator=tg).cuda()
    W1 = (torch.randn(64, 132, generator=tg) / 11).cuda()
    outs = []
    for dH in (G, G.float()):
        dW1, db1, dx = torch.empty(64, 132, device="cuda"), torch.empty(64, device="cuda"), torch.zeros(N, 64, device="cuda")
        yv.ops.edge_lin1_bwd_factorised(dH, x, g, W1, dW1, db1, dx=dx, dx_accumulate=True)
        outs.append((dW1, db1, dx))
    for a, b_ in zip(outs[0], outs[1]):
        assert float((a - b_).abs().max()) <= 1e-5 * float(b_.abs().max())


def test_bf16_storage_ops_round_to_nearest_even_and_reject_fp32_mixups():
    yv = _yv()
    N, E = 300, 1500
    rng = np.random.default_rng(0)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    g = yv.ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).cuda(),
                           torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32)).cuda(), None, N, 1)
    d_f = torch.randn(N, 64, device="cuda")
    dm32 = torch.empty(E, 64, device="cuda")
    dm16 = torch.empty(E, 64, device="cuda", dtype=torch.bfloat16)
    yv.ops.csr_mean_bwd(d_f, g, dm32)
    yv.ops.csr_mean_bwd(d_f, g, dm16)
    assert torch.equal(dm16, dm32.to(torch.bfloat16))                  # same rounding as torch's conversion
    out32, out16 = torch.zeros(N, 64, device="cuda"), torch.zeros(N, 64, device="cuda")
    yv.ops.csr_mean_fwd(dm16.float(), g, out32)
    yv.ops.csr_mean_fwd(dm16, g, out16)
    assert torch.equal(out32, out16)                                   # exact widening, same summation order
    with pytest.raises(ValueError):
        yv.ops.linear_fwd(dm16, torch.randn(64, 64, device="cuda"), None, torch.empty(E, 64, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("N,E", [(300, 1000), (4000, 30000)])
def test_fused_bn_csr_backward_bf16_storage_matches_fp32_on_the_same_values(N, E):
    """ops.BnCsrGrad with bfloat16-STORED Y / A / dA (bn_csr.hip, one-kernel form k_bn_csr_l2_bwd_h): the fp32
    instantiation run on the same (bf16-representable) values is the reference.  dgamma / dbeta / db are formed in fp32
    from the same values: fp32 summation noise.  The two products run on the bf16 matrix cores (round 4) like the
    forward Linear of this mode: dY, relu(bn(A)) and W are rounded to bfloat16 (2^-9 each) before dA = dY . W and
    dW = dY^T . A1, accumulation fp32 — dW within 8e-3 of its largest element and 5e-3 in norm (a sum of E products with
    independent 2^-8 errors; measured 4.3e-3 at E = 1000), dA within 2^-7 of its largest element (64 such products + the rounding of the stored output)."""
    import numpy as np
    yv = _yv()
    C = 64
    rng = np.random.default_rng(N + E)
    src = rng.integers(0, N, E); dst = np.sort(rng.integers(0, N, E))
    g = yv.ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).cuda(), torch.rand(E, 4).cuda(), None, N, 1)
    tg = torch.Generator().manual_seed(E)
    d_f = torch.randn(N, C, generator=tg).cuda()
    H2 = torch.randn(E, C, generator=tg).cuda().bfloat16()
    H1 = torch.randn(E, C, generator=tg).cuda().bfloat16()
    W = (torch.randn(C, C, generator=tg) / 8).cuda()
    c1 = torch.stack([torch.rand(C, generator=tg) + 0.5, torch.randn(C, generator=tg)]).cuda()
    gamma, beta = (torch.rand(C, generator=tg) + 0.5).cuda(), torch.randn(C, generator=tg).cuda()
    h2f = H2.float()
    mean, invstd = h2f.mean(0), 1 / torch.sqrt(h2f.var(0, unbiased=False) + 1e-5)
    scale = gamma * invstd
    coefs = torch.stack([scale, beta - mean * scale, mean, invstd]).contiguous()

    def run(Y, A, dt):
        dg, db = torch.empty(C).cuda(), torch.empty(C).cuda()
        dW, dbias, dA = torch.empty(C, C).cuda(), torch.empty(C).cuda(), torch.empty(E, C, dtype=dt).cuda()
        h = yv.ops.BnCsrGrad(d_f, g, Y, coefs[2], coefs[3], coefs[0], coefs[1], relu=True)
        h.stats(dg, db)
        h.bwd_w_and_x(A, W, dW, dbias, dA, a_pro=(c1[0], c1[1]), a_relu=True)
        return dg, db, dW, dbias, dA.float()
    ref = run(h2f, H1.float(), torch.float32)
    got = run(H2, H1, torch.bfloat16)
    for name, a, b in zip(("dgamma", "dbeta", "dW", "db"), ref[:4], got[:4]):
        tol = 2e-5 * (float(ref[4].abs().sum(0).max()) if name == "db" else max(float(a.abs().max()), 1e-6))
        if name == "dW":
            tol = 8e-3 * float(a.abs().max())
        assert float((a - b).abs().max()) <= tol, name
    assert float((ref[4] - got[4]).abs().max()) <= 2.0 ** -7 * float(ref[4].abs().max())
    rel = float((ref[2] - got[2]).norm() / ref[2].norm())
    assert rel <= 5e-3, rel
    again = run(H2, H1, torch.bfloat16)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# the edge stage on its own (yolat_edge_uv_mlp2_mean_eval_bf16): node tiles vs register-chained MFMA waves
# ---------------------------------------------------------------------------------------------
def _edge_stage_case(yv, n_props, nodes_lo, nodes_hi, seed, **kw):
    data, _ = yv.synth_batch(1, seed, num_proposals=n_props, nodes_lo=nodes_lo, nodes_hi=nodes_hi, **kw)
    N, P = int(data.x.shape[0]), int(data.bbox.shape[0])
    g = yv.ops.build_graph(data.edge.cuda(), data.e_attr.cuda(), data.bbox_idx.cuda(), N, P)
    gen = torch.Generator().manual_seed(seed)
    C = 64
    UV = torch.randn(N, 2 * C, generator=gen).to(torch.bfloat16).cuda()
    wc4 = (torch.randn(C, 4, generator=gen) * 2).cuda()
    s1 = (torch.rand(C, generator=gen) + 0.5).cuda()
    W2f = (torch.randn(C, C, generator=gen) / 8).to(torch.bfloat16).cuda()
    t2f = (torch.randn(C, generator=gen) * 0.3).cuda()
    root = torch.randn(N, C, generator=gen).cuda()
    return g, UV, wc4, s1, W2f, t2f, root


def _edge_stage_reference(g, UV, wc4, s1, W2f, t2f, root):
    """fp64 restatement of torch_vertex.py:330-337 on the factorised inputs, hidden activation rounded to bf16 (the
    one rounding both kernels share); returns (unrounded output, message scale)."""
    U, V = UV[:, :64].double(), UV[:, 64:].double()
    dst, src = g.dst.long(), g.src.long()
    z = U[dst] + V[src] + g.attr.double() @ (wc4.double() * s1.double()[:, None]).t()
    h1 = torch.relu(z).float().to(torch.bfloat16).double()
    m = torch.relu(h1 @ W2f.double().t() + t2f.double())
    N = U.shape[0]
    sums = torch.zeros(N, 64, dtype=torch.float64, device=U.device).index_add_(0, dst, m)
    deg = torch.bincount(dst, minlength=N).clamp(min=1).double()
    # (exact output, message scale, the most one bf16 rounding flip of a hidden activation can move a message)
    return root.double() + sums / deg[:, None], float(m.abs().max()), float(h1.abs().max() * W2f.double().abs().max()) * 2.0 ** -7


def _run_edge_stage(yv, g, UV, wc4, s1, W2f, t2f, root, variant):
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    N = UV.shape[0]
    out = torch.full((N, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    check(lib.yolat_edge_uv_mlp2_mean_eval_bf16(UV.data_ptr(), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                                g.row_ptr.data_ptr(), N, g.E, wc4.data_ptr(), s1.data_ptr(),
                                                W2f.data_ptr(), t2f.data_ptr(), root.data_ptr(), 64, out.data_ptr(), 64,
                                                variant, torch.cuda.current_stream().cuda_stream),
          "yolat_edge_uv_mlp2_mean_eval_bf16")
    return out


@pytest.mark.parametrize("shape", [
    dict(n_props=3000, nodes_lo=25, nodes_hi=25, edges_per_proposal=150),      # cfg-5-like: 6 in-edges per node
    dict(n_props=900, nodes_lo=3, nodes_hi=40, edge_factor=3.0),               # ragged, many nodes without in-edges
    dict(n_props=40, nodes_lo=30, nodes_hi=60, edges_per_proposal=3000),       # in-degree ~65: nodes span many steps
    dict(n_props=2500, nodes_lo=4, nodes_hi=30, edge_factor=1.2),              # ~1.2 edges per node: up to 16 ends per step
    dict(n_props=7, nodes_lo=5, nodes_hi=9, edge_factor=2.0),                  # a handful of edges: most waves idle
])
def test_edge_stage_bf16_chained_mfma_kernel_matches_reference_and_node_tiles(shape):
    """k_edge_chain_h (edge_chain.hip: layer 1 as identity-MFMAs on the gathered chunks, register-chained into layer 2,
    per-node running sums in registers) against the fp64 restatement and against the node-tile kernel: every output
    within one bf16 rounding of the exact value (2^-8 of its magnitude + the fp32 noise of the sum), every node
    written (incl. nodes without in-edges), bit-identical run to run."""
    yv = _yv()
    kw = dict(shape)
    args = _edge_stage_case(yv, kw.pop("n_props"), kw.pop("nodes_lo"), kw.pop("nodes_hi"), 7, **kw)
    g = args[0]
    want, mscale, flip = _edge_stage_reference(*args)
    tiles = _run_edge_stage(yv, *args, variant=1)
    if g.E < 16:
        pytest.skip("the chained kernel needs >= 16 edges")
    chain = _run_edge_stage(yv, *args, variant=2)
    again = _run_edge_stage(yv, *args, variant=2)
    assert torch.isfinite(chain.float()).all()
    assert torch.equal(chain.view(torch.int16), again.view(torch.int16))
    for name, got in (("node tiles", tiles), ("chained", chain)):
        d = (got.double() - want).abs()
        tol = want.abs() * 2.0 ** -8 + 2e-5 * mscale
        # a hidden activation whose fp32 pre-activation sits on a bf16 rounding boundary may round the other way than
        # in the fp64 restatement and move one message by up to `flip`: a few outputs per 100 000 (measured 8 of 4.8 M)
        # land beyond the one-rounding band, none beyond band + flip
        assert float((d > tol).float().mean()) < 2e-5, "%s: %d of %d outputs off by more than a bf16 rounding" % (
            name, int((d > tol).sum()), d.numel())
        assert not bool((d > tol + flip).any()), "%s: worst excess %.3e (flip bound %.3e)" % (
            name, float((d - tol).max()), flip)
    # the two kernels agree except where the exact value sits next to a bf16 rounding boundary
    differ = float((tiles.view(torch.int16) != chain.view(torch.int16)).float().mean())
    assert differ < 0.02, differ


@pytest.mark.parametrize("shape", [
    dict(n_props=8000, nodes_lo=25, nodes_hi=25, edges_per_proposal=150),      # cfg 5: N = 200 k, E = 1.2 M
    dict(n_props=8000, nodes_lo=4, nodes_hi=40, edge_factor=1.2),              # cfg-3-like (ragged, ~1.2 edges per node), chain forced on
])
def test_edge_chain_kernel_soak_50_runs_bit_identical_and_exact(shape):
    """k_edge_chain_h carries two workarounds for code-generation hazards (edge_chain.hip:55-72: an inline-asm v_max on MFMA
    results that the hazard recogniser does not see; v_pk_fma_f32 with op_sel reading the wrong half of an 8-byte LDS read)
    — both showed up as run-to-run DIFFERENT sums in a few nodes per launch at E = 1.2 M.  The guard used to be a soak script
    outside the suite; here: 50 launches at full cfg-5 size and 50 on a ragged cfg-3-like graph with the chained kernel
    forced (variant 2), every launch bit-identical to the first, and the first within one bf16 rounding of the fp64
    restatement (same bounds as the test above)."""
    yv = _yv()
    kw = dict(shape)
    args = _edge_stage_case(yv, kw.pop("n_props"), kw.pop("nodes_lo"), kw.pop("nodes_hi"), 19, **kw)
    g = args[0]
    if shape["nodes_lo"] == 25:
        assert g.E == 1200000 and args[1].shape[0] == 200000
    first = _run_edge_stage(yv, *args, variant=2)
    ref_bits = first.view(torch.int16).clone()
    bad_runs = 0
    for _ in range(49):
        out = _run_edge_stage(yv, *args, variant=2)
        bad_runs += int(not torch.equal(out.view(torch.int16), ref_bits))
    assert bad_runs == 0, "%d of 49 repeat launches differ from the first" % bad_runs
    want, mscale, flip = _edge_stage_reference(*args)
    d = (first.double() - want).abs()
    tol = want.abs() * 2.0 ** -8 + 2e-5 * mscale
    assert torch.isfinite(first.float()).all()
    assert float((d > tol).float().mean()) < 2e-5 and not bool((d > tol + flip).any())


@pytest.mark.gpu
@pytest.mark.parametrize("M,pro", [(70001, True), (65536, False), (131072 + 33, True)])
def test_linear64_bf16_row_stream_is_bit_identical_to_the_tile_kernel(M, pro):
    """k_hlin64_stream (bf16_linear.hip, round 4; taken by yolat_linear_fwd_h for K = Nout = 64, M >= 65536: the second edge
    Linear of a bf16-storage training conv layer, torch_vertex.py:331 nn.3) against the hgemm tile kernel run on row ranges
    below the threshold (48 000 rows: a multiple of 32, the statistics' group size): bf16 outputs and fp32 (sum, M2)
    statistics BIT-identical, ragged last tile included; fp64 check of the product on the widened values."""
    yv = _yv()
    ops = yv.ops
    gen = torch.Generator().manual_seed(M)
    A = torch.randn(M, 64, generator=gen).cuda().bfloat16()
    W = (torch.randn(64, 64, generator=gen) / 8).cuda()
    b = torch.randn(64, generator=gen).cuda()
    sc = (torch.rand(64, generator=gen) + 0.5).cuda() if pro else None
    sh = torch.randn(64, generator=gen).cuda() * 0.3 if pro else None
    apro = (sc, sh) if pro else None
    Y = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    st = ops.stats_buffer(M, 64, A.device)
    st.fill_(float("nan"))
    ops.linear_fwd(A, W, b, Y, a_pro=apro, a_relu=pro, stats=st)
    parts_y, parts_s = [], []
    for lo in range(0, M, 48000):
        hi = min(lo + 48000, M)
        Yp = torch.zeros(hi - lo, 64, device="cuda", dtype=torch.bfloat16)
        sp = ops.stats_buffer(hi - lo, 64, A.device)
        ops.linear_fwd(A[lo:hi], W, b, Yp, a_pro=apro, a_relu=pro, stats=sp)
        parts_y.append(Yp)
        parts_s.append(sp.view(-1)[:2 * 64 * ((hi - lo + 31) // 32)])
    assert torch.equal(Y, torch.cat(parts_y))
    assert torch.equal(st.view(-1)[:2 * 64 * ((M + 31) // 32)], torch.cat(parts_s))
    Ain = A.double()
    if pro:
        Ain = torch.relu(A.float() * sc + sh).bfloat16().double()
    ref = Ain @ W.bfloat16().double().t() + b.double()
    assert float((Y.double() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
