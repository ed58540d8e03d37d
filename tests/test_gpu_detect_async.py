"""GPU tests of the asynchronous detection: SparseCADGCN.detect_submit / DetectHandle, evaluation.detect_batch_async and
detect_stream over yolat_detect (csrc/detect.hip).  The reference of every case is the synchronous path of the same build —
evaluation.detect_batch = predict -> ops.detect_scores -> non_max_suppression_batched — and the comparison is torch.equal:
the submission enqueues the same selection, the same fp32 steps and the same NMS, it only never reads a size back."""
import copy
import time

import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_detect import _eval_loader, _i32

pytestmark = pytest.mark.gpu


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _model(yv, optkw, seed):
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), seed).cuda().eval()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape and g.shape[1] == 6
        assert torch.equal(g, w)


def _items(yv, seed, n, n_classes=17, num_proposals=14, nodes_hi=9, sized=True):
    out = []
    for i in range(n):
        it = yv.synth_graph(num_proposals=num_proposals + 3 * i, nodes_lo=4, nodes_hi=nodes_hi, edge_factor=1.5,
                            n_classes=n_classes, seed=seed * 100 + i, with_roots=True)
        if sized:
            it.width = torch.tensor([1000.0 + 10 * i])
            it.height = torch.tensor([800.0 - 10 * i])
        out.append(it)
    return out


def _shift_last_class(model, data, slices, how):
    """move the last class's bias so that it is the arg-max of no root ("none"), of every proposal ("all") or of about
    half of them ("half", the shift of test_predict_one_submission_equals_the_two_pass_extraction)"""
    with torch.no_grad():
        z = model(data, slices)[0]
        gap = z[:, :-1].max(1).values - z[:, -1]
        d = {"half": float(gap.median()), "all": float(gap.max()) + 0.5, "none": float(gap.min()) - 0.5}[how]
        model.prediction_cls[2][0].bias[model.n_classes - 1] += d
    data._yolat_stage = None


# ---------------------------------------------------------------------------------------------
# 1. bit-equality with the synchronous path
# ---------------------------------------------------------------------------------------------
def test_submit_result_equals_detect_batch_on_the_detect_fixture():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    batch = _eval_loader(yv, 6)[1]
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    h = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    assert isinstance(h, yv.DetectHandle)
    got = h.result()
    assert h.ready() and h.result() is got
    assert len(got) == 2 and all(g.shape[0] > 0 for g in got)
    _same(got, want)
    assert float(got[0][:, :4].max()) > 1.0                      # pixels, not the unit square
    # the method itself, on a batch the caller has fixed up
    data, slices = copy.deepcopy(batch)
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same(model.detect_submit(data, slices, conf_thres=0.05, iou_thres=0.5).result(), want)


def test_rows_kernel_equals_predict_plus_detect_scores():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    data, slices = copy.deepcopy(_eval_loader(yv, 6)[1])
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    with torch.no_grad():
        out = model.predict(data, slices)
        logits, bbox = model(data, slices)
    ptr = [int(v) for v in out[4]]
    scale = torch.tensor([[1000.0, 800.0, 1000.0, 800.0]] * 2).cuda()
    want = yv.ops.detect_scores(out[0].float(), out[1].float().contiguous(), _i32(ptr), scale)
    h = model.detect_submit(data, slices, conf_thres=0.05, iou_thres=0.5)
    sel, pred = h.sel, h.pred
    total = int(sel[0])
    R_cap = sel.numel() - (4 + 2 + 1)
    assert total == want.shape[0] == ptr[-1] and pred.shape == (R_cap, 4 + 3) and total <= R_cap
    assert [int(v) for v in sel[4:7]] == ptr
    got = yv.ops.detect_rows(logits, bbox.float().contiguous(), sel, 2, R_cap, scale)
    assert torch.equal(got[:total], want) and torch.equal(pred[:total], want)
    assert not bool(got[total:].any()) and not bool(pred[total:].any())          # spare rows: zeros
    plain = yv.ops.detect_rows(logits, bbox.float().contiguous(), sel, 2, R_cap, scale, softmax=False)
    want_plain = yv.ops.detect_scores(out[0].float(), out[1].float().contiguous(), _i32(ptr), scale, softmax=False)
    assert torch.equal(plain[:total], want_plain)
    h.result()


def test_batched_nms_takes_rows_that_belong_to_no_image():
    """yolat_nms_batched with R > image_ptr[B]: the rows behind the last image are non-candidates of image B and sort behind
    every image's own range — the detections are those of the call on the first image_ptr[B] rows (what yolat_detect
    relies on), whatever the spare rows hold"""
    yv = _yv()
    rng = np.random.default_rng(5)
    R, nc, spare = 700, 4, 333
    pred = torch.from_numpy(rng.random((R + spare, 5 + nc)).astype(np.float32)).cuda()
    pred[:, 2:4] = pred[:, 0:2] + 0.05 + 0.2 * pred[:, 2:4]
    pred[:, :4] *= 500.0
    ptr = _i32([0, 250, 250, 700])
    want_det, want_cnt = yv.ops.nms_batched(pred[:R].contiguous(), ptr, 0.1, 0.5)
    got_det, got_cnt = yv.ops.nms_batched(pred, ptr, 0.1, 0.5)
    assert torch.equal(got_cnt, want_cnt) and torch.equal(got_det, want_det)
    assert int(want_cnt[0]) > 0 and int(want_cnt[1]) == 0 and int(want_cnt[2]) > 0


# ---------------------------------------------------------------------------------------------
# 2. the spare-row edge
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["none", "all"])
def test_no_child_selected_and_every_child_selected(how):
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    data, slices = copy.deepcopy(_eval_loader(yv, 6)[1])
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _shift_last_class(model, data, slices, how)
    want = yv.detect_batch(model, data, slices, conf_thres=0.01, iou_thres=0.5, fixup=False)
    h = model.detect_submit(data, slices, conf_thres=0.01, iou_thres=0.5)
    sel = h.sel.cpu()
    R = len(data.roots)
    Ctot = sum(len(r.children) for r in data.roots)
    assert Ctot > 0 and sel.numel() == 4 + 3 + R + Ctot
    assert int(sel[0]) == (R if how == "none" else R + Ctot)      # the regime: Ctot spare rows / none
    got = h.result()
    _same(got, want)
    assert sum(g.shape[0] for g in got) > 0


# ---------------------------------------------------------------------------------------------
# 3. tile edges: R_cap beyond one 256-row block, candidates per image beyond one 1024-candidate chunk of the walk
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile_case():
    yv = _yv()
    data, slices = yv.synth_batch(3, 21, num_proposals=300, nodes_lo=4, nodes_hi=30, edge_factor=1.3, with_roots=True)
    model = _model(yv, dict(n_classes=17, n_blocks=2, n_blocks_out=2), 3)
    _shift_last_class(model, data, slices, "half")
    return yv, model, data, slices


@pytest.mark.parametrize("conf_thres,agnostic", [(0.0, False), (0.25, False), (0.0, True)])
def test_tile_edges(tile_case, conf_thres, agnostic):
    yv, model, data, slices = tile_case
    want = yv.detect_batch(model, data, slices, conf_thres=conf_thres, iou_thres=0.45, agnostic=agnostic, fixup=False)
    h = model.detect_submit(data, slices, conf_thres=conf_thres, iou_thres=0.45, agnostic=agnostic)
    sel, pred = h.sel.cpu(), h.pred
    R = len(data.roots)
    R_cap = sel.numel() - (4 + 3 + 1)
    total = int(sel[0])
    assert R_cap > 256 and R < total < R_cap                      # some, not all, children: spare rows exist
    if conf_thres == 0.0:
        ptr = [int(v) for v in sel[4:8]]
        obj, cls = pred[:, 4:5], pred[:, 5:]
        cand = ((obj > 0) & (obj * cls > 0)).sum(1).cpu()
        per_image = [int(cand[ptr[i]:ptr[i + 1]].sum()) for i in range(3)]
        assert min(per_image) > 1024, per_image                   # more than one chunk of k_det_nms per image
    got = h.result()
    _same(got, want)
    assert all(g.shape[0] > 0 for g in got)


# ---------------------------------------------------------------------------------------------
# 4. smallest shapes
# ---------------------------------------------------------------------------------------------
def test_one_image():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    batch = yv.collate(_items(yv, 31, 1, n_classes=3))
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5).result()
    assert len(got) == 1 and got[0].shape[0] > 0
    _same(got, want)


def test_two_classes_one_nms_class():
    yv = _yv()
    model = _model(yv, dict(gu.PREDICT_OPT, n_classes=2), 5)
    batch = yv.collate(_items(yv, 32, 2, n_classes=2))
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5).result()
    _same(got, want)
    assert sum(g.shape[0] for g in got) > 0 and all(float(g[:, 5].abs().max()) == 0.0 for g in got if g.shape[0])


def test_an_image_without_roots_between_two_others():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    items = _items(yv, 33, 3, n_classes=3)
    both = yv.collate(copy.deepcopy(items))
    items[1].roots = []
    batch = yv.collate(items)
    assert [int(v) for v in batch[1]["roots"]][1] == [int(v) for v in batch[1]["roots"]][2]
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5).result()
    _same(got, want)
    assert tuple(got[1].shape) == (0, 6) and got[0].shape[0] > 0 and got[2].shape[0] > 0
    full = yv.detect_batch_async(model, *both, conf_thres=0.05, iou_thres=0.5).result()
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])      # the neighbours do not notice


# ---------------------------------------------------------------------------------------------
# 5. other model forms
# ---------------------------------------------------------------------------------------------
def test_sigmoid_classifier_model():
    yv = _yv()
    model = _model(yv, dict(gu.PREDICT_OPT, classifier="sigmoid"), 5)
    batch = _eval_loader(yv, 6)[1]
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5, classifier="sigmoid")
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5, classifier="sigmoid").result()
    _same(got, want)
    assert sum(g.shape[0] for g in got) > 0
    data, slices = copy.deepcopy(batch)
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same(model.detect_submit(data, slices, conf_thres=0.05, iou_thres=0.5).result(), want)      # default: the model's own


def test_bf16_eval_precision():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    model.set_eval_precision("bf16")
    batch = _eval_loader(yv, 6)[1]
    want = yv.detect_batch(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5)
    got = yv.detect_batch_async(model, *copy.deepcopy(batch), conf_thres=0.05, iou_thres=0.5).result()
    _same(got, want)
    assert sum(g.shape[0] for g in got) > 0


# ---------------------------------------------------------------------------------------------
# 6. in flight
# ---------------------------------------------------------------------------------------------
def test_four_batches_in_flight_collected_in_reverse_order():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    batches = _eval_loader(yv, 11) + _eval_loader(yv, 12)
    want = [yv.detect_batch(model, *copy.deepcopy(b), conf_thres=0.05, iou_thres=0.5) for b in batches]
    runs = []
    for _ in range(2):
        handles = [yv.detect_batch_async(model, *copy.deepcopy(b), conf_thres=0.05, iou_thres=0.5) for b in batches]
        got = [None] * 4
        for i in (3, 2, 1, 0):
            got[i] = handles[i].result()
        for g, w in zip(got, want):
            _same(g, w)
        runs.append(got)
    for a, b in zip(*runs):
        _same(a, b)
    assert len({tuple(g.shape[0] for g in got_b) for got_b in runs[0]}) > 1       # four different batches


# ---------------------------------------------------------------------------------------------
# 7. submit does not wait for the device
# ---------------------------------------------------------------------------------------------
SLEEP_CYCLES = 200_000_000


def test_submit_returns_while_the_device_is_still_busy():
    """A spin of SLEEP_CYCLES on the stream, an event behind it, then detect_submit: the event has not completed when submit
    returns, and nothing was read from the device; result() reads once.
    Measured on the MI355X (event timing): torch.cuda._sleep(200 000 000) holds the stream for 85.8 ms (1 000 000 cycles:
    1.6 ms, 10 000 000: 4.2 ms); one warm detect_submit of this batch takes 0.14 - 0.17 ms of host time in a loop of twenty
    (median 0.150 ms) and 0.32 ms inside this test — the spin is 270 to 570 times one submit, where the test needs ten.
    The test measures both again and asserts the factor before it trusts the query.  (Nothing sleeps on the host:
    result() synchronises with the spin.)"""
    yv = _yv()
    if getattr(torch.cuda, "_sleep", None) is None:
        pytest.skip("torch.cuda._sleep is not available")
    model = _model(yv, gu.PREDICT_OPT, 5)
    data, slices = yv.collate_to_device(_items(yv, 34, 2, n_classes=3))
    want = yv.detect_batch(model, data, slices, conf_thres=0.05, iou_thres=0.5, fixup=False)
    yv.detect_batch_async(model, data, slices, conf_thres=0.05, iou_thres=0.5, fixup=False).result()      # warm: caches, allocator
    torch.cuda.synchronize()
    start, busy = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reads0 = yv.ops.D2H_READS
    start.record()
    torch.cuda._sleep(SLEEP_CYCLES)
    busy.record()
    t0 = time.perf_counter()
    h = yv.detect_batch_async(model, data, slices, conf_thres=0.05, iou_thres=0.5, fixup=False)
    submit_ms = (time.perf_counter() - t0) * 1e3
    still_busy = not busy.query()
    assert yv.ops.D2H_READS == reads0                            # no read during submit
    assert not h.ready()
    got = h.result()
    assert yv.ops.D2H_READS == reads0 + 1                        # exactly one in result()
    spin_ms = start.elapsed_time(busy)
    print("spin %.1f ms, submit %.3f ms of host time" % (spin_ms, submit_ms))
    assert spin_ms >= 10.0 * submit_ms
    assert still_busy
    _same(got, want)


# ---------------------------------------------------------------------------------------------
# 8. fall-back and status
# ---------------------------------------------------------------------------------------------
def test_a_doctored_tree_between_two_good_batches_takes_the_synchronous_path():
    yv = _yv()
    model = _model(yv, dict(n_classes=17, n_blocks=2, n_blocks_out=2), 4)
    kw = dict(num_proposals=120, nodes_lo=4, nodes_hi=20, edge_factor=1.3, with_roots=True)
    good1, bad, good2 = yv.synth_batch(1, 25, **kw), yv.synth_batch(1, 23, **kw), yv.synth_batch(2, 26, **kw)
    root, nxt = bad[0].roots[0], bad[0].roots[1]
    assert nxt.value["idx_pos"][0] >= root.value["idx_pos"][1]
    root.value["idx_pos"] = (root.value["idx_pos"][0], nxt.value["idx_pos"][1])       # a range over TWO proposals
    opts = dict(conf_thres=0.05, iou_thres=0.5, fixup=False)
    want1, want2 = yv.detect_batch(model, *good1, **opts), yv.detect_batch(model, *good2, **opts)
    calls = []
    orig = model._predict_two_pass
    model._predict_two_pass = lambda d, s: calls.append(1) or orig(d, s)
    reads0 = yv.ops.D2H_READS
    try:
        h1 = yv.detect_batch_async(model, *good1, **opts)
        hb = yv.detect_batch_async(model, *bad, **opts)
        h2 = yv.detect_batch_async(model, *good2, **opts)
        assert calls == [] and yv.ops.D2H_READS == reads0        # nothing decided at submit
        try:
            out = hb.result()
            assert len(out) == 1
        except (KeyError, IndexError, ValueError):
            pass          # what the two-pass extraction makes of such a tree (test_predict_falls_back_when_the_tree_is_...)
        assert calls == [1]
        assert int(hb.sel[1]) != 0
        _same(h2.result(), want2)
        _same(h1.result(), want1)
        assert calls == [1]
    finally:
        del model._predict_two_pass
    # the model is not left condemned: the next submission is clean
    _same(yv.detect_batch_async(model, *good1, **opts).result(), want1)


def test_a_malformed_batch_raises_at_result_what_the_forward_check_raises():
    yv = _yv()
    model = _model(yv, dict(n_classes=17, n_blocks=2, n_blocks_out=2), 4)
    kw = dict(num_proposals=40, nodes_lo=4, nodes_hi=12, edge_factor=1.3, with_roots=True)
    good = yv.synth_batch(1, 27, **kw)
    bad = yv.synth_batch(1, 28, **kw)
    bad[0].edge = bad[0].edge.clone()
    bad[0].edge[0, 0] = bad[0].x.shape[0] + 5                     # a node id outside [0, N)
    opts = dict(conf_thres=0.05, iou_thres=0.5, fixup=False)
    want = yv.detect_batch(model, *good, **opts)
    hb = yv.detect_batch_async(model, *bad, **opts)
    hg = yv.detect_batch_async(model, *good, **opts)
    with pytest.raises(IndexError, match="edge_index"):
        hb.result()
    _same(hg.result(), want)                                     # each handle carries the flags of its own forward


def test_a_prepared_graph_batch_raises_at_submit():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    data, slices = yv.collate_to_device(_items(yv, 35, 2, n_classes=3), csr=True)
    with pytest.raises(ValueError, match="csr=False"):
        model.detect_submit(data, slices)
    with pytest.raises(ValueError, match="csr=False"):
        yv.detect_batch_async(model, data, slices, fixup=False)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.detect_submit(*yv.collate_to_device(_items(yv, 35, 2, n_classes=3)))
    model.eval()


# ---------------------------------------------------------------------------------------------
# 9. loader
# ---------------------------------------------------------------------------------------------
def _loader_lists(yv, n):
    return [_items(yv, 50 + i, 1 + i % 3, num_proposals=9 + 5 * (i % 4), nodes_hi=9 + 2 * (i % 3)) for i in range(n)]


def test_detect_stream_over_a_device_loader_and_over_a_list_of_batches():
    yv = _yv()
    model = _model(yv, dict(n_classes=17, n_blocks=2, n_blocks_out=2), 13)
    lists = _loader_lists(yv, 7)
    opts = dict(conf_thres=0.05, iou_thres=0.5)
    want = [yv.detect_batch(model, *yv.collate_to_device(items), fixup=False, **opts) for items in lists]
    assert sum(w.shape[0] for ws in want for w in ws) > 0
    loader = yv.DeviceLoader(lists, slots=4, csr=False)
    got = list(yv.detect_stream(model, loader, depth=2, **opts))
    loader.close()
    assert len(got) == len(want) == 7
    for g, w in zip(got, want):
        _same(g, w)
    for depth in (1, 4, 16):
        got = list(yv.detect_stream(model, [yv.collate_to_device(items) for items in lists], depth=depth, **opts))
        assert len(got) == 7
        for g, w in zip(got, want):
            _same(g, w)
    loader = yv.DeviceLoader(lists, slots=4, csr=False)
    with pytest.raises(ValueError, match="slots"):
        next(yv.detect_stream(model, loader, depth=3, **opts))
    loader.close()


def test_fallback_of_a_loader_batch_whose_ring_slot_has_been_rewritten():
    """two slots, three draws: the first batch's slot holds the third batch by the time its handle is asked — the fall-back
    collates the batch again from the host items the lazy batch keeps"""
    yv = _yv()
    model = _model(yv, dict(n_classes=17, n_blocks=2, n_blocks_out=2), 13)
    lists = _loader_lists(yv, 3)
    first = lists[0][0]
    root, nxt = first.roots[0], first.roots[1]
    assert nxt.value["idx_pos"][0] >= root.value["idx_pos"][1]
    root.value["idx_pos"] = (root.value["idx_pos"][0], nxt.value["idx_pos"][1])
    opts = dict(conf_thres=0.05, iou_thres=0.5, fixup=False)

    def sync(items):
        try:
            return yv.detect_batch(model, *yv.collate_to_device(items), **opts)
        except (KeyError, IndexError, ValueError) as e:
            return type(e)

    want = [sync(items) for items in lists]
    loader = yv.DeviceLoader(lists, slots=2, csr=False)
    handles = [yv.detect_batch_async(model, data, slices, **opts) for data, slices in loader]
    assert len(handles) == 3 and int(handles[0].sel[1]) != 0
    for h, w in zip(handles, want):
        if isinstance(w, type):
            with pytest.raises(w):
                h.result()
        else:
            _same(h.result(), w)
    loader.close()
