"""GPU tests of the asynchronous evaluation: SparseCADGCN.evaluate_submit / EvalHandle, evaluation.evaluate_batch_async,
evaluate_stream and test(opt.async_eval) over yolat_evaluate (csrc/evaluate.hip).  The reference of every case is the
synchronous path of the same build — evaluation.evaluate_batch(device_post=True) = predict -> DetectionLoss -> arg-max ->
detect_post_device — and the comparison is equality, the loss included: the submission enqueues the same selection, the
same row code of the loss in the same fixed-order trees, the same scores, NMS and true-positive walk; it only never reads
a size back.  The rows kernel is also compared per element with DetectionLoss / torch on the gathered rows."""
import copy
import math
import time
import types

import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_detect import _eval_loader
from test_gpu_detect_async import _items, _shift_last_class

pytestmark = pytest.mark.gpu


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _model(yv, optkw, seed):
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), seed).cuda().eval()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a)).tobytes()


def _same_rep(got, want, K):
    """the dict of an EvalHandle against evaluate_batch's: everything equal, floats bit for bit"""
    assert got["labels"] == want["labels"]
    assert (got["n_true"], got["n_total"]) == (want["n_true"], want["n_total"])
    for k in ("y_pred", "y_true"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape == (want["n_total"],)
        np.testing.assert_array_equal(got[k], want[k])
    assert set(got["loss"]) == set(want["loss"]) == {"loss", "loss_cls"}
    for k in ("loss", "loss_cls"):
        g, w = got["loss"][k], want["loss"][k]
        assert isinstance(g, float) and ((math.isnan(g) and math.isnan(w)) or _bits(np.float32(g)) == _bits(np.float32(w))), (g, w)
    assert len(got["sample_metrics"]) == len(want["sample_metrics"])
    for mg, mw in zip(got["sample_metrics"], want["sample_metrics"]):
        assert len(mg) == len(mw)
        for (tpg, sg, lg), (tpw, sw, lw) in zip(mg, mw):
            assert tpg.dtype == np.float64 and tpg.shape == tpw.shape == (len(sw),)
            np.testing.assert_array_equal(tpg, tpw)
            assert _bits(sg) == _bits(sw) and _bits(lg) == _bits(lw)
    conf = got["confusion"]
    assert conf.dtype == np.int64 and conf.shape == (K, K)
    np.testing.assert_array_equal(conf, _yv().confusion_counts(got["y_true"], got["y_pred"], K))
    in_range = int(((got["y_true"] >= 0) & (got["y_true"] < K)).sum())
    assert int(conf.sum()) == in_range and int(np.trace(conf)) == got["n_true"]


def _sync(yv, model, batch, classifier="softmax", fixup=True, **kw):
    crit = yv.DetectionLoss(yv.Opt(classifier=classifier))
    with torch.no_grad():
        return yv.evaluate_batch(model, crit, *batch, classifier=classifier, fixup=fixup, device_post=True, **kw)


def _with_targets(items, n_classes, seed, empty=()):
    """the fields the evaluation loop reads on top of _items': up to six targets per image (none for the images in `empty`)"""
    rng = np.random.default_rng(seed)
    for i, it in enumerate(items):
        P = it.bbox.shape[0]
        k = 0 if i in empty else min(6, P)
        pick = rng.choice(P, size=k, replace=False)
        it.gt_bbox = it.bbox[pick].clone()
        it.gt_labels = torch.from_numpy(rng.integers(0, max(n_classes - 1, 1), size=k)).long()
        it.has_obj = torch.ones(P, dtype=torch.long)
    return items


def _eval_items(yv, seed, n, n_classes=3, empty=(), **kw):
    return _with_targets(_items(yv, seed, n, n_classes=n_classes, **kw), n_classes, seed, empty)


# ---------------------------------------------------------------------------------------------
# 1. - 3. equality with the synchronous path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["softmax", "sigmoid", "bf16"])
def test_result_equals_evaluate_batch_with_device_post(form):
    yv = _yv()
    classifier = "sigmoid" if form == "sigmoid" else "softmax"
    model = _model(yv, dict(gu.PREDICT_OPT, classifier=classifier), 5)
    if form == "bf16":
        model.set_eval_precision("bf16")
    K = gu.PREDICT_OPT["n_classes"]
    loader = _eval_loader(yv, 4)
    for batch in loader:
        want = _sync(yv, model, copy.deepcopy(batch), classifier)
        data, slices = copy.deepcopy(batch)
        h = yv.evaluate_batch_async(model, data, slices, classifier=classifier)
        assert isinstance(h, yv.EvalHandle)
        got = h.result()
        assert h.ready() and h.result() is got
        _same_rep(got, want, K)
        assert got["n_total"] > 0 and math.isfinite(got["loss"]["loss"]) and len(got["sample_metrics"]) == 10
        assert sum(len(m[0]) for m in got["sample_metrics"][0]) > 0
        # the caller's batch keeps its labels and its proposal offsets (evaluate_batch overwrites both)
        assert torch.equal(data.labels, batch[0].labels) and torch.equal(slices["bbox"], batch[1]["bbox"])
    # the method itself with the model's own classifier, on a batch the caller has fixed up
    data, slices = copy.deepcopy(loader[1])
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    _same_rep(model.evaluate_submit(data, slices).result(), want, K)


def test_detect_submit_and_evaluate_submit_leave_the_same_selection_and_detections():
    """the two submissions share their front half and yolat_detect: on one batch, with evaluate_submit's thresholds, the
    record of the selection up to its last row, the detection counts and the detections are the same bytes"""
    yv = _yv()
    K = 17
    model = _model(yv, dict(n_classes=K, n_blocks=2, n_blocks_out=2), 4)
    data, slices = yv.collate_to_device(_eval_items(yv, 81, 2, n_classes=K, num_proposals=40, nodes_hi=12))
    _shift_last_class(model, data, slices, "half")
    hd = model.detect_submit(data, slices, conf_thres=0.0, iou_thres=0.5)
    he = model.evaluate_submit(data, slices)
    torch.cuda.synchronize()
    total = int(hd.sel[0])
    words = yv.ops.sel_words(2, total)
    assert 0 < len(data.roots) <= total <= hd.sel.numel() - yv.ops.sel_words(2, 0)      # every root, children of some
    assert _bits(hd.sel[:words].cpu()) == _bits(he.sel[:words].cpu())
    det, det_count = he.device_record()[:2]
    assert int(det_count.sum()) > 0
    assert _bits(hd.det_count.cpu()) == _bits(det_count.cpu()) and _bits(hd.det.cpu()) == _bits(det.cpu())
    hd.result(), he.result()


# ---------------------------------------------------------------------------------------------
# 4. the rows kernel at workgroup edges, per element against DetectionLoss / torch on the gathered rows
# ---------------------------------------------------------------------------------------------
def _select(yv, model, data, slices, logits, bbox):
    """yolat_predict_select on `logits` -> the sel record (device int32) and R_cap"""
    import ctypes
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    ep, se, sc, bp, N, E, P, dev = yv.submit.predict_operands(model, data, logits, bbox)
    t, ft, _ = yv.submit.predict_tree(data, slices, dev)
    R, Ctot, B = ft["R"], ft["Ctot"], ft["B"]
    sel = torch.empty(4 + B + 1 + R + Ctot, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.yolat_predict_select_workspace_bytes(N, P, R)) + 16, dtype=torch.uint8, device=dev)
    check(lib.yolat_predict_select(logits.data_ptr(), logits.stride(0), P, logits.shape[1], ep if E > 0 else None, se, sc,
                                   bp, N, E, ctypes.byref(t), sel.data_ptr(), ws.data_ptr(), ws.numel(), yv.ops._stream()),
          "yolat_predict_select")
    torch.cuda.synchronize()
    return sel, ft


@pytest.mark.parametrize("regime", ["none", "all", 256, 257])
def test_rows_kernel_at_workgroup_edges(regime):
    yv = _yv()
    K = 17
    model = _model(yv, dict(n_classes=K, n_blocks=2, n_blocks_out=2), 4)
    items = _items(yv, 61, 3, n_classes=K, num_proposals=100)
    assert [it.bbox.shape[0] for it in items] == [100, 103, 106]
    data, slices = yv.collate_to_device(items)
    if regime in ("none", "all"):
        _shift_last_class(model, data, slices, regime)
    with torch.no_grad():
        logits, bbox = model(data, slices)
    logits = logits.float().contiguous().clone()
    from yolat_vectorgraphicsrecognition_amd import data as D
    ft = D.flatten_tree(data, slices)
    R, Ctot = ft["R"], ft["Ctot"]
    R_cap = R + Ctot
    assert R_cap == 309 > 256 > R
    if isinstance(regime, int):
        # the last class is made the arg-max of exactly the roots whose children bring the row count to `regime`
        counts = np.diff(ft["child_ptr"])
        left, chosen = regime - R, []
        for i, c in enumerate(counts):
            if 0 < c <= left:
                chosen.append(i)
                left -= int(c)
        assert left == 0, "no subset of the roots' child counts reaches %d" % regime
        rows = torch.from_numpy(ft["root_row"].astype(np.int64)).cuda()
        top, low = logits.max() + 1.0, logits.min() - 1.0
        logits[rows, K - 1] = low
        logits[rows[torch.tensor(chosen)], K - 1] = top
    sel, _ = _select(yv, model, data, slices, logits, bbox)
    total = int(sel[0])
    assert int(sel[1]) == 0
    assert total == {"none": R, "all": R_cap}.get(regime, regime)
    picked = sel[4 + 3 + 1:4 + 3 + 1 + total].long()
    labels = data.labels
    assert labels.is_cuda and labels.dtype == torch.int64
    for classifier in ("softmax", "sigmoid"):
        z = logits if classifier == "softmax" else yv.ops.sigmoid(logits)
        loss, stats, y_pred, y_true = yv.ops.eval_rows(z, labels, sel, 3, R_cap, softmax=classifier == "softmax")
        rows_z, rows_y = z[picked].contiguous(), labels[picked].contiguous()      # what yolat_predict_gather gathers
        with torch.no_grad():
            want = yv.DetectionLoss(yv.Opt(classifier=classifier))((rows_z,), types.SimpleNamespace(labels=rows_y))["loss"]
        assert math.isfinite(float(want)) and _bits(loss.cpu().numpy()[0]) == _bits(want.cpu().numpy()), (float(loss), float(want))
        want_pred = rows_z.max(1)[1]
        assert torch.equal(y_pred[:total].long(), want_pred) and torch.equal(y_true[:total].long(), rows_y)
        stats = stats.cpu().numpy()
        assert stats[0] == int((want_pred == rows_y).sum()) and stats[1] == total
        np.testing.assert_array_equal(stats[2:].reshape(K, K),
                                      yv.confusion_counts(rows_y.cpu().numpy(), want_pred.cpu().numpy(), K))
        # a second run is bit-identical (fixed-order trees, integer atomics)
        loss2, stats2, _, _ = yv.ops.eval_rows(z, labels, sel, 3, R_cap, softmax=classifier == "softmax")
        assert torch.equal(loss2, loss) and np.array_equal(stats2.cpu().numpy(), stats)


def test_rows_kernel_arg_max_takes_the_first_maximum_and_a_nan_as_the_maximum():
    yv = _yv()
    K, P = 5, 6
    z = torch.tensor([[0.0, 2.0, 2.0, 1.0, 2.0],                    # a tie: the first index
                      [1.0, float("nan"), 3.0, float("nan"), 0.0],  # a NaN is the maximum, the first one
                      [float("nan"), 9.0, 9.0, 9.0, 9.0],
                      [-1.0, -2.0, -3.0, -0.5, -0.5],
                      [float("-inf")] * 4 + [0.0],
                      [3.0, 3.0, 3.0, 3.0, 3.0]], device="cuda")
    labels = torch.tensor([1, 1, 0, 3, 4, 2], device="cuda")
    sel = torch.tensor([P, 0, 0, 0, 0, P] + list(range(P)), dtype=torch.int32, device="cuda")
    loss, stats, y_pred, y_true = yv.ops.eval_rows(z, labels, sel, 1, P)
    want = z.max(1)[1]
    assert want.tolist() == [1, 1, 0, 3, 4, 0]
    assert torch.equal(y_pred.long(), want) and torch.equal(y_true.long(), labels)
    assert int(stats[0]) == 5 and int(stats[1]) == P and math.isnan(float(loss))


# ---------------------------------------------------------------------------------------------
# 5. the smallest and the largest class count; one beyond
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 32])
def test_smallest_and_largest_class_count(K):
    yv = _yv()
    model = _model(yv, dict(gu.PREDICT_OPT, n_classes=K), 5)
    items = _eval_items(yv, 71, 2, n_classes=K)
    want = _sync(yv, model, yv.collate(copy.deepcopy(items)))
    got = yv.evaluate_batch_async(model, *yv.collate(copy.deepcopy(items))).result()
    _same_rep(got, want, K)
    assert got["n_total"] > 0


def test_one_class_beyond_the_rows_kernel_takes_the_synchronous_loop():
    yv = _yv()
    K = 33
    model = _model(yv, dict(gu.PREDICT_OPT, n_classes=K), 5)
    loader = [yv.collate(_eval_items(yv, 72 + b, 2, n_classes=K)) for b in range(2)]
    data, slices = copy.deepcopy(loader[0])
    with pytest.raises(ValueError, match="K in"):
        yv.evaluate_batch_async(model, data, slices)
    torch.cuda.synchronize()
    opt = yv.Opt(**dict(gu.PREDICT_OPT, n_classes=K))
    opt.device_postprocess = True
    want = yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt), opt)
    opt_a = yv.Opt(**dict(gu.PREDICT_OPT, n_classes=K))
    opt_a.device_postprocess = True
    opt_a.async_eval = True
    got = yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt_a), opt_a)
    assert got == want and opt_a.test_report["map"] == opt.test_report["map"]
    assert "confusion" not in opt_a.test_report


# ---------------------------------------------------------------------------------------------
# 6. image and label edge cases
# ---------------------------------------------------------------------------------------------
def test_an_image_without_roots_and_an_image_without_targets():
    yv = _yv()
    model = _model(yv, gu.PREDICT_OPT, 5)
    items = _eval_items(yv, 73, 3, empty=(2,))
    items[1].roots = []
    batch = yv.collate(copy.deepcopy(items))
    assert [int(v) for v in batch[1]["roots"]][1] == [int(v) for v in batch[1]["roots"]][2]
    assert [int(v) for v in batch[1]["gt_labels"]][2] == [int(v) for v in batch[1]["gt_labels"]][3]
    want = _sync(yv, model, copy.deepcopy(batch))
    got = yv.evaluate_batch_async(model, *copy.deepcopy(batch)).result()
    _same_rep(got, want, 3)
    first = got["sample_metrics"][0]
    assert len(first) == 3 and len(first[0][0]) > 0 and len(first[1][0]) == 0 and len(first[2][0]) > 0
    assert all(float(m[2][0].sum()) == 0.0 for m in got["sample_metrics"])      # no target: no true positive


# ---------------------------------------------------------------------------------------------
# 7. the label guard
# ---------------------------------------------------------------------------------------------
def test_host_labels_out_of_range_raise_at_submit_and_device_labels_poison_the_loss():
    yv = _yv()
    K = 3
    model = _model(yv, gu.PREDICT_OPT, 5)
    items = _eval_items(yv, 74, 2)
    first_root = items[0].roots[0].value["idx_bbox"]              # a row every selection keeps
    data, slices = yv.collate(copy.deepcopy(items))
    data.labels = data.labels.clone()
    data.labels[first_root] = K
    reads0 = yv.ops.D2H_READS
    with pytest.raises(IndexError, match="out of bounds"):
        yv.evaluate_batch_async(model, data, slices)
    assert yv.ops.D2H_READS == reads0
    clean = yv.evaluate_batch_async(model, *yv.collate_to_device(copy.deepcopy(items)), fixup=False).result()
    assert math.isfinite(clean["loss"]["loss"])
    data, slices = yv.collate_to_device(copy.deepcopy(items))
    data.labels[first_root] = K
    got = yv.evaluate_batch_async(model, data, slices, fixup=False).result()
    assert math.isnan(got["loss"]["loss"]) and math.isnan(got["loss"]["loss_cls"])
    assert got["n_total"] == clean["n_total"] and int(got["confusion"].sum()) == got["n_total"] - 1
    where = np.flatnonzero(got["y_true"] == K)
    assert where.shape == (1,)
    np.testing.assert_array_equal(got["y_pred"], clean["y_pred"])
    dropped = clean["confusion"].copy()
    dropped[clean["y_true"][where[0]], clean["y_pred"][where[0]]] -= 1
    np.testing.assert_array_equal(got["confusion"], dropped)      # the other rows' counts are intact
    data, slices = yv.collate_to_device(copy.deepcopy(items))
    data.labels[first_root] = K
    _same_rep(got, _sync(yv, model, (data, slices), fixup=False), K)


# ---------------------------------------------------------------------------------------------
# 8. submit does not wait for the device
# ---------------------------------------------------------------------------------------------
SLEEP_CYCLES = 200_000_000


def test_submit_returns_while_the_device_is_still_busy():
    """the arrangement of test_gpu_detect_async's test of the same name: a spin on the stream, an event behind it, then
    evaluate_submit — the event has not completed when submit returns and nothing was read from the device; result() reads
    exactly once"""
    yv = _yv()
    if getattr(torch.cuda, "_sleep", None) is None:
        pytest.skip("torch.cuda._sleep is not available")
    model = _model(yv, gu.PREDICT_OPT, 5)
    items = _eval_items(yv, 75, 2)
    want = _sync(yv, model, yv.collate_to_device(copy.deepcopy(items)), fixup=False)
    data, slices = yv.collate_to_device(items)
    yv.evaluate_batch_async(model, data, slices, fixup=False).result()      # warm: caches, allocator, the upload
    torch.cuda.synchronize()
    start, busy = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reads0 = yv.ops.D2H_READS
    start.record()
    torch.cuda._sleep(SLEEP_CYCLES)
    busy.record()
    t0 = time.perf_counter()
    h = yv.evaluate_batch_async(model, data, slices, fixup=False)
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
    _same_rep(got, want, 3)


# ---------------------------------------------------------------------------------------------
# 9. fall-back
# ---------------------------------------------------------------------------------------------
def _doctor(item):
    root, nxt = item.roots[0], item.roots[1]
    assert nxt.value["idx_pos"][0] >= root.value["idx_pos"][1]
    root.value["idx_pos"] = (root.value["idx_pos"][0], nxt.value["idx_pos"][1])       # a range over TWO proposals


def _sync_or_exception(yv, model, items):
    try:
        return _sync(yv, model, yv.collate_to_device(copy.deepcopy(items)), fixup=False)
    except (KeyError, IndexError, ValueError) as e:
        return type(e)          # what the two-pass extraction makes of such a tree


def test_a_doctored_tree_between_two_good_batches_takes_the_synchronous_path():
    yv = _yv()
    K = 17
    model = _model(yv, dict(n_classes=K, n_blocks=2, n_blocks_out=2), 4)
    kw = dict(n_classes=K, num_proposals=40, nodes_hi=12)
    good1, bad, good2 = _eval_items(yv, 81, 1, **kw), _eval_items(yv, 82, 1, **kw), _eval_items(yv, 83, 2, **kw)
    _doctor(bad[0])
    want1, wantb, want2 = (_sync_or_exception(yv, model, it) for it in (good1, bad, good2))
    calls = []
    orig = model._predict_two_pass
    model._predict_two_pass = lambda d, s: calls.append(1) or orig(d, s)
    reads0 = yv.ops.D2H_READS
    try:
        h1, hb, h2 = (yv.evaluate_batch_async(model, *yv.collate_to_device(copy.deepcopy(it)), fixup=False)
                      for it in (good1, bad, good2))
        assert calls == [] and yv.ops.D2H_READS == reads0        # nothing decided at submit
        flagged = int(hb.sel[1])
        assert flagged != 0
        if isinstance(wantb, type):
            with pytest.raises(wantb):
                hb.result()
        else:
            _same_rep(hb.result(), wantb, K)
        assert calls == [1]
        _same_rep(h2.result(), want2, K)
        _same_rep(h1.result(), want1, K)
        assert calls == [1]
    finally:
        del model._predict_two_pass
    # the model is not left condemned: the next submission is clean
    _same_rep(yv.evaluate_batch_async(model, *yv.collate_to_device(copy.deepcopy(good1)), fixup=False).result(), want1, K)


def test_fallback_of_a_loader_batch_whose_ring_slot_has_been_rewritten():
    """two slots, three draws: the first batch's slot holds the third batch by the time its handle is asked — the fall-back
    collates the batch again from the host items the lazy batch keeps"""
    yv = _yv()
    K = 17
    model = _model(yv, dict(n_classes=K, n_blocks=2, n_blocks_out=2), 13)
    lists = [_eval_items(yv, 84 + i, 1 + i % 2, n_classes=K, num_proposals=12 + 5 * i, nodes_hi=9 + 2 * i) for i in range(3)]
    _doctor(lists[0][0])
    want = [_sync_or_exception(yv, model, items) for items in lists]
    loader = yv.DeviceLoader(copy.deepcopy(lists), slots=2, csr=False)
    handles = [yv.evaluate_batch_async(model, data, slices, fixup=False) for data, slices in loader]
    assert len(handles) == 3 and int(handles[0].sel[1]) != 0
    for h, w in zip(handles, want):
        if isinstance(w, type):
            with pytest.raises(w):
                h.result()
        else:
            _same_rep(h.result(), w, K)
    loader.close()


# ---------------------------------------------------------------------------------------------
# 10. the stream driver
# ---------------------------------------------------------------------------------------------
def _stream_lists(yv, n, K):
    return [_eval_items(yv, 90 + i, 1 + i % 3, n_classes=K, num_proposals=9 + 5 * (i % 4), nodes_hi=9 + 2 * (i % 3))
            for i in range(n)]


def test_evaluate_stream_depths_streams_and_loader():
    yv = _yv()
    K = 17
    model = _model(yv, dict(n_classes=K, n_blocks=2, n_blocks_out=2), 13)
    lists = _stream_lists(yv, 6, K)
    want = [_sync(yv, model, yv.collate_to_device(copy.deepcopy(items)), fixup=False) for items in lists]
    assert sum(w["n_total"] for w in want) > 0 and len({w["n_total"] for w in want}) > 1
    three = [torch.cuda.Stream() for _ in range(3)]
    for depth in (1, 3):
        for streams in (None, three[:1], three):
            batches = [yv.collate_to_device(copy.deepcopy(items)) for items in lists]
            got = list(yv.evaluate_stream(model, batches, depth=depth, streams=streams))
            assert len(got) == 6
            for g, w in zip(got, want):
                _same_rep(g, w, K)
    torch.cuda.synchronize()
    for streams in (None, three[:1]):
        loader = yv.DeviceLoader(copy.deepcopy(lists), slots=6, csr=False)
        got = list(yv.evaluate_stream(model, loader, depth=3, streams=streams))
        loader.close()
        assert len(got) == 6
        for g, w in zip(got, want):
            _same_rep(g, w, K)
    loader = yv.DeviceLoader(copy.deepcopy(lists), slots=6, csr=False)
    with pytest.raises(ValueError, match="one stream"):
        next(yv.evaluate_stream(model, loader, depth=3, streams=three))
    with pytest.raises(ValueError, match="slots"):
        next(yv.evaluate_stream(model, loader, depth=5))
    loader.close()


# ---------------------------------------------------------------------------------------------
# 11. the evaluation loop
# ---------------------------------------------------------------------------------------------
def test_evaluate_with_async_eval_returns_what_the_synchronous_loop_returns():
    yv = _yv()
    K = gu.PREDICT_OPT["n_classes"]
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**gu.PREDICT_OPT)), 5).cuda()
    loader = _eval_loader(yv, 3)

    def run(**attrs):
        opt = yv.Opt(**gu.PREDICT_OPT)
        opt.device_postprocess = True
        for k, v in attrs.items():
            setattr(opt, k, v)
        return yv.evaluate(model, copy.deepcopy(loader), yv.DetectionLoss(opt), opt), opt.test_report

    want, ref = run()
    assert want is not None and "confusion" not in ref
    runs = [run(async_eval=True), run(async_eval=True), run(async_eval=True, eval_depth=2, eval_streams=2)]
    for got, rep in runs:
        assert got == want
        assert rep["map"] == ref["map"] and rep["map_all"] == ref["map_all"] and rep["top1"] == ref["top1"]
        assert rep["loss"] == ref["loss"]                         # the mean of bit-equal per-batch values
        conf = rep["confusion"]
        assert conf.dtype == np.int64 and conf.shape == (K, K) and int(conf.sum()) > 0
        assert int(np.trace(conf)) / int(conf.sum()) == rep["top1"]
        np.testing.assert_array_equal(conf, runs[0][1]["confusion"])

    class Other(yv.DetectionLoss):      # any other criterion: the synchronous loop, with that criterion
        pass

    opt = yv.Opt(**gu.PREDICT_OPT)
    opt.device_postprocess = True
    opt.async_eval = True
    assert yv.evaluate(model, copy.deepcopy(loader), Other(opt), opt) == want and "confusion" not in opt.test_report
