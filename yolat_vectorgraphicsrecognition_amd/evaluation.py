"""The reference's evaluation loop (cad_recognition/train.py:324-508, ``test``) on the device path: per batch the
index fix-up, the two-pass ``model.predict``, the loss, top-1 accuracy, and per image
softmax -> [1 - P(last class), P(other classes)] -> class-aware NMS -> true-positive statistics at the IoU
thresholds 0.5 .. 0.95; then AP per class and threshold.  Same inputs (``(data, slices)`` batches of collated items
with ``labels, has_obj, gt_bbox, gt_labels, width, height`` next to the graph tensors) and the same value written to
``opt.test_value`` / returned (the mean AP at the LAST threshold, train.py:507-508); the intermediate numbers the
reference only logs are returned in ``opt.test_report``."""
from collections import deque

import numpy as np
import torch

from .data import fixup_offsets, DeviceLoader
from . import ops
from .submit import EvalHandle, image_scales
from .postprocess import (non_max_suppression, get_batch_statistics, ap_per_class, detect_post_device,
                          non_max_suppression_batched)


def _prepare(data, slices, fixup):
    """what every per-batch entry starts with: the index fix-up (train.py:346-366) unless the batch carries its offsets
    already, and the ``edge_control`` attribute of the reference's loop"""
    if fixup:
        fixup_offsets(data, slices)
    if not hasattr(data, "edge_control"):
        data.edge_control = None


def evaluate_batch(model, criterion, data, slices, classifier="softmax", iou_thresholds=None, conf_thres=0.0,
                   iou_thres=0.5, fixup=True, device_post=False):
    """One iteration of the loop (train.py:343-460).  Returns a dict: per-threshold ``sample_metrics`` (lists of
    [true_positives, scores, labels] per image), the ground-truth ``labels`` list, ``loss`` dict, ``n_true`` /
    ``n_total`` of the top-1 accuracy, ``y_pred`` / ``y_true``.
    device_post=True: scores, NMS and the true-positive walk of ALL images and thresholds run as three device calls
    (postprocess.detect_post_device, csrc/detect.hip) between one upload and one read-back, instead of per image from
    Python; same detections and flags, the softmax may differ from torch's in the last bit."""
    if iou_thresholds is None:
        iou_thresholds = np.linspace(0.5, 0.95, 10)
    _prepare(data, slices, fixup)
    out = model.predict(data, slices)
    keep = torch.as_tensor([int(v) for v in out[3]], dtype=torch.long)
    data.labels = data.labels[keep]
    if hasattr(data, "has_obj"):
        data.has_obj = data.has_obj[keep]
    slices["bbox"] = out[4]
    loss = criterion(out, data)
    pred_cls, pred_coord = out[0], out[1].clone()
    pred_label = pred_cls.max(1)[1]
    truth = data.labels.to(pred_label.device)
    rep = {"loss": {k: float(v) for k, v in loss.items()}, "n_true": int((pred_label == truth).sum()),
           "n_total": int(pred_label.shape[0]), "y_pred": pred_label.cpu().numpy(), "y_true": data.labels.cpu().numpy(),
           "sample_metrics": [[] for _ in iou_thresholds], "labels": []}
    image_ptr, label_ptr = slices["bbox"], slices["gt_labels"]
    if device_post:
        scales, gts = [], []
        for i in range(len(image_ptr) - 1):
            w, h = float(data.width[i]), float(data.height[i])
            scale = torch.tensor([w, h, w, h], dtype=torch.float32)
            gt = data.gt_bbox[int(label_ptr[i]):int(label_ptr[i + 1])].float() * scale
            gl = data.gt_labels[int(label_ptr[i]):int(label_ptr[i + 1])]
            rep["labels"] += gl.tolist()
            scales.append(scale)
            gts.append(torch.cat((gl.float().unsqueeze(1), gt), 1))
        rep["sample_metrics"] = detect_post_device(
            pred_cls.detach().float(), pred_coord.float().contiguous(), image_ptr, torch.stack(scales).numpy(),
            torch.cat(gts, 0).numpy(), label_ptr, iou_thresholds, softmax=classifier == "softmax", conf_thres=conf_thres,
            iou_thres=iou_thres)
        return rep
    for i in range(len(image_ptr) - 1):
        pc = pred_cls[image_ptr[i]:image_ptr[i + 1]]
        pb = pred_coord[image_ptr[i]:image_ptr[i + 1]]
        w, h = float(data.width[i]), float(data.height[i])
        scale = torch.tensor([w, h, w, h], dtype=pb.dtype, device=pb.device)
        gt = data.gt_bbox[int(label_ptr[i]):int(label_ptr[i + 1])].float() * scale.cpu()
        gl = data.gt_labels[int(label_ptr[i]):int(label_ptr[i + 1])]
        targets = torch.cat((torch.zeros(gl.shape[0], 1), gl.float().unsqueeze(1), gt), 1)
        rep["labels"] += gl.tolist()
        if classifier == "softmax":
            pc = torch.softmax(pc, dim=1)
        conf = torch.cat((1 - pc[:, -1:], pc[:, :-1]), 1)
        pred = torch.cat((pb * scale, conf), 1).unsqueeze(0)
        outputs = [o.cpu() for o in non_max_suppression(pred, conf_thres=conf_thres, iou_thres=iou_thres)]
        for t, th in enumerate(iou_thresholds):
            rep["sample_metrics"][t] += get_batch_statistics(outputs, targets, iou_threshold=th)
    return rep


def detect_batch(model, data, slices, conf_thres=0.25, iou_thres=0.45, classifier="softmax", agnostic=False, fixup=True):
    """Inference on one collated batch, the loop of the reference's detect.py: ``model.predict``, then scores and the
    class-aware NMS of all images as two device calls (ops.detect_scores, postprocess.non_max_suppression_batched).
    Returns one device tensor [k, 6] = (x1, y1, x2, y2, conf, cls) per image, boxes in pixels of the image
    (``data.width`` / ``data.height``; without them the boxes stay in the model's unit square)."""
    _prepare(data, slices, fixup)
    with torch.no_grad():
        out = model.predict(data, slices)
    logits, boxes, image_ptr = out[0].detach().float(), out[1].detach().float().contiguous(), out[4]
    B = len(image_ptr) - 1
    scales = image_scales(data, B)
    dev = logits.device
    ptr = torch.as_tensor([int(v) for v in image_ptr], dtype=torch.int32)
    up = torch.from_numpy(np.concatenate([ptr.numpy(), scales.reshape(-1).view(np.int32)])).to(dev)
    pred = ops.detect_scores(logits, boxes, up[:B + 1], up[B + 1:].view(torch.float32).view(B, 4), classifier == "softmax")
    return non_max_suppression_batched(pred, ptr, conf_thres=conf_thres, iou_thres=iou_thres, agnostic=agnostic)


def detect_batch_async(model, data, slices, conf_thres=0.25, iou_thres=0.45, classifier="softmax", agnostic=False,
                       fixup=True):
    """``detect_batch`` as a submission: the same ``fixup`` / ``edge_control`` handling, then
    ``model.detect_submit`` — forward, selection, scores and NMS enqueued on the current stream, nothing read back.
    Returns the ``DetectHandle``; ``handle.result()`` is the list ``detect_batch`` returns, bit for bit."""
    _prepare(data, slices, fixup)
    return model.detect_submit(data, slices, conf_thres=conf_thres, iou_thres=iou_thres, agnostic=agnostic,
                               classifier=classifier)


def detect_stream(model, batches, depth=4, **kw):
    """Generator over the detections of ``batches`` — a ``DeviceLoader(..., csr=False)`` or any iterable of
    ``(data, slices)`` device batches (``collate_to_device(items)``) — with up to ``depth`` batches in flight on the
    current stream: batch i + depth is submitted before the host looks at batch i, so the device never waits for a host
    read.  Yields, in order, what ``detect_batch`` returns for each batch.  ``kw``: the keywords of
    ``detect_batch_async``; ``fixup`` defaults to False here (device batches carry their offsets already).
    A DeviceLoader hands out ring slots.  A submission enqueues everything that reads its batch before the next draw
    (the ring rule of the loader's docstring), and a handle's fall-back collates the batch again from its host items, so
    no handle reads a slot that has been rewritten; the batches the handles in flight hold are valid for ``slots - 1``
    further draws, one of which is the draw in progress: ``depth <= slots - 2`` is required (ValueError otherwise, also
    when the loader does not say how many slots it has)."""
    depth = int(depth)
    if depth < 1:
        raise ValueError("detect_stream needs depth >= 1")
    _check_loader_depth("detect_stream", batches, depth)
    kw.setdefault("fixup", False)
    yield from _in_flight(_submissions(model, batches, None, kw, detect_batch_async), depth)


def confusion_counts(y_true, y_pred, K):
    """Confusion matrix np.int64 [K, K] of two equally long integer sequences: entry [t, p] counts the rows of true class t
    predicted as p (the table train.py:489-505 prints).  Rows whose true or predicted class is outside [0, K) are ignored."""
    t = np.asarray(y_true, dtype=np.int64).reshape(-1)
    p = np.asarray(y_pred, dtype=np.int64).reshape(-1)
    if t.shape != p.shape:
        raise ValueError("confusion_counts expects y_true and y_pred of one length")
    ok = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    out = np.zeros((int(K), int(K)), dtype=np.int64)
    np.add.at(out, (t[ok], p[ok]), 1)
    return out


def evaluate_batch_async(model, data, slices, fixup=True, **kw):
    """``evaluate_batch(device_post=True)`` as a submission: the same ``fixup`` / ``edge_control`` handling, then
    ``model.evaluate_submit`` — forward, selection, loss, top-1 and confusion counts, scores, NMS and the true-positive
    walk enqueued on the current stream, nothing read back.  Returns the ``EvalHandle``; ``handle.result()`` is the dict
    ``evaluate_batch`` returns (the loss bit for bit) plus ``confusion``.  ``kw``: ``iou_thresholds``, ``conf_thres``,
    ``iou_thres``, ``classifier`` (default: the model's own).  ``data.labels`` and ``slices["bbox"]`` are left as they
    are; the criterion is DetectionLoss' by construction."""
    _prepare(data, slices, fixup)
    return model.evaluate_submit(data, slices, **kw)


class EpochMetrics(object):
    """The metrics of an evaluation epoch accumulated ON THE DEVICE (csrc/metrics.hip): every ``EvalHandle`` is appended to
    one epoch record without being read, and ``result()`` brings the epoch home in one copy.

    ``EpochMetrics(model, iou_thresholds, capacity_images=1024)``: 1 to 32 thresholds (one bit of a slot's mask each), a
    model of 2 to 32 classes.  The record starts at ``capacity_images`` images and grows — allocate, device copy, swap, no
    read — when the epoch holds more.

    ``add(handle)``  takes the handle WITHOUT calling its ``result()``: one ``yolat_metrics_append`` launch on the handle's
        stream behind its last launch, slots and batch number assigned here on the host (so the record is the same for one
        stream and for four), an event, and a non-blocking copy of the batch's two flags into pinned memory.  No blocking
        call.  Later calls poll the events (a query, never a wait) and let go of every handle whose flags arrived as
        zero; a handle with a flag set is kept for ``result()``.  Returns the batch's number.
    ``result()``  the current stream waits for every stream's last append; ONE flags read if a handle is still pending; a
        batch whose forward flagged its input raises what ``ops.check_status_word`` raises; a batch with the tree flag goes
        through ``EvalHandle._fallback`` and its outcome is uploaded into the batch's reserved slots
        (``ops.metrics_append_host``); then ``yolat_metrics_finalize`` and ONE device -> host copy.  Returns the report
        of ``test()`` — ``iou_thresholds``, ``map`` (per threshold the mean AP over the classes with targets, 0.0 without
        any), ``map_all`` (their sum / 10, as the reference divides), ``top1``, ``loss``, ``confusion`` — plus ``ap``
        [T, K], ``p``, ``r``, ``classes`` (the ids with targets), ``n_gt`` and ``n_p`` [K]; None when no batch was added.
        A target class that is not an integer in [0, K) raises ValueError.
    Score ties keep epoch order (image, then detection rank): ``np.argsort(-conf, kind="stable")``."""

    MIN_BATCH_CAP = 256

    def __init__(self, model, iou_thresholds, capacity_images=1024):
        ths = np.asarray(iou_thresholds, dtype=np.float64).reshape(-1)
        T, K = int(ths.shape[0]), int(getattr(model, "n_classes", 0))
        if not 1 <= T <= ops.METRICS_MAX_THRESHOLDS:
            raise ValueError("EpochMetrics takes 1 to %d IoU thresholds, got %d" % (ops.METRICS_MAX_THRESHOLDS, T))
        if not 2 <= K <= ops.METRICS_MAX_CLASSES:
            raise ValueError("EpochMetrics takes a model of 2 to %d classes, got %d" % (ops.METRICS_MAX_CLASSES, K))
        if int(capacity_images) < 1:
            raise ValueError("EpochMetrics needs capacity_images >= 1")
        self.model, self.iou_thresholds, self.T, self.K = model, ths, T, K
        self.capacity_images = int(capacity_images)
        from collections import deque
        self._rec, self._retired, self._pinned = None, [], None
        self._n_images = self._n_batches = 0
        self._pending, self._flagged = deque(), []
        self._last = {}              # raw stream -> (stream object, event behind its last append)
        self._ready, self._ready_id, self._seen = None, 0, {}     # the record's last reset / growth and who waited for it
        self._result = None
        self.grown = 0

    # -- the record ------------------------------------------------------------------------------
    def _reserve(self, n_images, n_batches, device, stream):
        """a record that holds n_images / n_batches, made or grown on `stream`; the other streams wait for it in add()"""
        rec = self._rec
        if rec is not None and n_images <= rec.capacity_images and n_batches <= rec.batch_cap:
            return rec
        if rec is None:
            cap, bcap = max(self.capacity_images, n_images), max(self.MIN_BATCH_CAP, n_batches)
            new = ops.metrics_record(cap, self.K, bcap, device)
        else:
            cap, bcap = rec.capacity_images, rec.batch_cap
            while cap < n_images:
                cap *= 2
            while bcap < n_batches:
                bcap *= 2
            for s, ev in self._last.values():          # every append into the old record is in front of the copy
                stream.wait_event(ev)
            new = ops.metrics_grow(rec, cap, bcap)
            self._retired.append(rec)                  # alive until result(): other streams may still be writing it
            self.grown += 1
        if self._pinned is None or self._pinned.shape[0] < new.batch_cap:
            self._pinned = torch.zeros((new.batch_cap, 2), dtype=torch.int32).pin_memory()
        self._ready = torch.cuda.Event()
        self._ready.record(stream)
        self._ready_id += 1
        self._seen = {}
        self._rec = new
        return new

    def _poll(self):
        while self._pending and self._pending[0][3].query():
            h, b, base, _, flags = self._pending.popleft()
            if flags[b, 0] != 0 or flags[b, 1] != 0:
                self._flagged.append((h, b, base, int(flags[b, 1])))

    def add(self, handle):
        if not isinstance(handle, EvalHandle):
            raise TypeError("EpochMetrics.add takes the EvalHandle of evaluate_submit / evaluate_batch_async")
        if self._result is not None:
            raise RuntimeError("EpochMetrics.result() has closed this epoch: make a new EpochMetrics for the next one")
        if handle.T != self.T or handle.K != self.K:
            raise ValueError("the handle was submitted with %d thresholds and %d classes, the epoch holds %d and %d"
                             % (handle.T, handle.K, self.T, self.K))
        self._poll()
        B, stream = handle.B, handle.stream
        key = stream.cuda_stream
        base, b = self._n_images, self._n_batches
        with torch.cuda.stream(stream):
            rec = self._reserve(base + B, b + 1, handle.device, stream)
            if self._seen.get(key) != self._ready_id:
                stream.wait_event(self._ready)
                rec.buf.record_stream(stream)
                self._seen[key] = self._ready_id
            det, det_count, tp, stats, loss = handle.device_record()
            ops.metrics_append(rec, det, det_count, tp, stats, loss, handle.gt_label, handle.sel, base, b)
            pinned = self._pinned
            pinned[b].copy_(rec.batch_flags()[b], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._n_images, self._n_batches = base + B, b + 1
        self._last[key] = (stream, ev)
        self._pending.append((handle, b, base, ev, pinned.numpy()))
        return b

    def _upload_fallback(self, handle, b, base):
        """the synchronous evaluation of a batch whose tree was flagged -> its reserved slots"""
        res = handle._fallback()
        B, T = handle.B, handle.T
        det = np.zeros((B, ops.MAX_DET, 6), dtype=np.float32)
        cnt = np.zeros(B, dtype=np.int32)
        tp = np.zeros((T, B, ops.MAX_DET), dtype=np.uint8)
        for t in range(T):
            for i, (flags, scores, labels) in enumerate(res["sample_metrics"][t]):
                k = len(flags)
                cnt[i] = k
                det[i, :k, 4], det[i, :k, 5] = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.float32)
                tp[t, i, :k] = np.asarray(flags) != 0
        stats = np.concatenate([[res["n_true"], res["n_total"]], np.asarray(res["confusion"]).reshape(-1)]).astype(np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(handle.device)
        ops.metrics_append_host(self._rec, up(det), up(cnt), up(tp), up(stats),
                                up(np.asarray([res["loss"]["loss"]], dtype=np.float32)),
                                up(np.asarray(res["labels"], dtype=np.float32).reshape(-1)), base, b)

    def result(self):
        if self._result is not None:
            return self._result
        if self._n_batches == 0:
            return None
        cur = ops.current_stream_object()
        for s, ev in self._last.values():
            cur.wait_event(ev)
        cur.wait_event(self._ready)
        rec, nb = self._rec, self._n_batches
        rec.buf.record_stream(cur)
        self._poll()
        flagged = list(self._flagged)
        if self._pending:
            flags = ops.d2h(rec.batch_flags()[:nb]).numpy()           # the one flags read
            flagged += [(h, b, base, int(flags[b, 1])) for h, b, base, _, _ in self._pending if flags[b].any()]
        self._pending.clear()
        for h, b, base, status in sorted(flagged, key=lambda e: e[1]):
            if status != 0:
                ops.check_status_word(torch.tensor([status], dtype=torch.int32))   # raises for every flag a forward sets
            self._upload_fallback(h, b, base)        # the device left the batch's slots unfilled
        self._flagged = []
        out = ops.metrics_finalize(rec, self._n_images, nb, self.T)
        m = ops.metrics_unpack(ops.d2h(out).numpy(), self.T, self.K, nb)     # the one copy that brings the epoch home
        self._retired = []
        if m["status"] & ops.METRICS_BAD_GT_LABEL:
            raise ValueError("gt_labels hold a class id that is not an integer in [0, %d) (YOLAT_METRICS_BAD_GT_LABEL)"
                             % self.K)
        K = self.K
        classes = np.flatnonzero(m["n_gt"] > 0)
        maps = [float(np.mean(m["ap"][t, classes])) if len(classes) else 0.0 for t in range(self.T)]
        stats = m["stats"]
        rep = {"iou_thresholds": self.iou_thresholds, "map": maps, "top1": int(stats[0]) / max(int(stats[1]), 1),
               "loss": {"loss": m["loss_mean"], "loss_cls": m["loss_mean"]},
               "confusion": stats[2:].reshape(K, K).astype(np.int64), "map_all": float(np.sum(maps) / 10),
               "ap": m["ap"], "p": m["p"], "r": m["r"], "classes": classes.astype("int32"), "n_gt": m["n_gt"],
               "n_p": m["n_p"], "batch_flags": m["batch_flags"]}
        self._result = rep
        return rep


MAX_EVAL_STREAMS = 4


def _submissions(model, batches, streams, kw, submit):
    """The handles of ``submit(model, data, slices, **kw)`` — evaluate_batch_async or detect_batch_async — in batch order,
    nothing read; the three ways to submit: on the current stream (streams None); a DeviceLoader under streams[0], the draws
    included (the loader hands a slot back behind an event on the drawing stream); batch i under streams[i % n], behind an
    event recorded on the caller's stream after the batch was drawn.  Every listed stream first waits for the caller's
    stream at entry.  A handle is yielded outside its stream's ``with`` block: it is read under the caller's stream."""
    if streams is None:
        for data, slices in batches:
            yield submit(model, data, slices, **kw)
        return
    home = ops.current_stream_object()
    entry = torch.cuda.Event()
    entry.record(home)
    for s in streams:
        s.wait_event(entry)
    if isinstance(batches, DeviceLoader):
        it = iter(batches)
        while True:
            with torch.cuda.stream(streams[0]):
                nxt = next(it, None)
                if nxt is None:
                    break
                h = submit(model, nxt[0], nxt[1], **kw)
            yield h
        return
    for i, (data, slices) in enumerate(batches):
        s = streams[i % len(streams)]
        drawn = torch.cuda.Event()
        drawn.record(home)
        s.wait_event(drawn)
        with torch.cuda.stream(s):
            h = submit(model, data, slices, **kw)
        yield h


def _in_flight(handles, depth):
    """``result()`` of every handle in order, handle i + depth drawn (= submitted) before handle i is read"""
    flying = deque()
    for h in handles:
        flying.append(h)
        if len(flying) >= depth:
            yield flying.popleft().result()
    while flying:
        yield flying.popleft().result()


def _check_loader_depth(name, batches, depth):
    """over a DeviceLoader: depth <= slots - 2 (detect_stream's docstring says why)"""
    if isinstance(batches, DeviceLoader):
        slots = getattr(batches, "_slots", None)
        if not isinstance(slots, int):
            raise ValueError("%s cannot tell how many slots the loader has" % name)
        if depth > slots - 2:
            raise ValueError("%s(depth=%d) over a DeviceLoader needs slots >= depth + 2, the loader has %d"
                             % (name, depth, slots))


def evaluate_stream(model, batches, depth=4, streams=None, **kw):
    """Generator over the evaluation dicts of ``batches`` — a ``DeviceLoader(..., csr=False)`` or any iterable of
    ``(data, slices)`` batches — with up to ``depth`` batches in flight: batch i + depth is submitted before the host looks
    at batch i.  Yields, in order, what ``evaluate_batch_async(...).result()`` returns for each batch.  ``kw``: the
    keywords of ``evaluate_batch_async``; ``fixup`` defaults to False here (device batches carry their offsets already).
    ``streams``: None — the current stream — or a list of 1 to 4 ``torch.cuda.Stream``: batch i is submitted under
    ``streams[i % len(streams)]``, so that the serial chains of consecutive batches overlap on the GPU.  Every listed
    stream first waits for an event recorded on the caller's current stream at entry, and each submission for one
    recorded there after its batch was drawn (a batch collated while the generator runs is complete before another stream
    reads it).  A handle's tensors are allocated under its stream and only host arrays leave the generator.
    Over a DeviceLoader: ``depth <= slots - 2`` as for ``detect_stream``, and one stream at the most — the loader's ring
    belongs to the stream its batches are drawn on (ValueError otherwise).
    ``metrics`` (a keyword of its own among ``kw``, default None): an ``EpochMetrics`` — every submitted handle goes to ``metrics.add`` instead of being read, and the
    generator yields the batch's number in the epoch; ``metrics.result()`` then is the epoch's report.  The same loader and
    stream rules; nothing limits the batches in flight but the polling of ``add``."""
    depth = int(depth)
    metrics = kw.pop("metrics", None)
    if depth < 1:
        raise ValueError("evaluate_stream needs depth >= 1")
    if streams is not None:
        streams = list(streams)
        if not 1 <= len(streams) <= MAX_EVAL_STREAMS:
            raise ValueError("evaluate_stream takes 1 to %d streams, got %d" % (MAX_EVAL_STREAMS, len(streams)))
        if isinstance(batches, DeviceLoader) and len(streams) > 1:
            raise ValueError("evaluate_stream over a DeviceLoader takes one stream: the loader's ring belongs to the stream "
                             "its batches are drawn on")
    _check_loader_depth("evaluate_stream", batches, depth)
    kw.setdefault("fixup", False)
    if metrics is not None and not isinstance(metrics, EpochMetrics):
        raise TypeError("evaluate_stream(metrics=) takes an EpochMetrics")
    handles = _submissions(model, batches, streams, kw, evaluate_batch_async)
    if metrics is not None:
        for h in handles:
            yield metrics.add(h)
    else:
        yield from _in_flight(handles, depth)


def _async_eval_applies(model, criterion, opt):
    """test() takes evaluate_stream when opt.async_eval is set, the criterion is DetectionLoss itself (what the rows stage
    computes) and the class count is one the rows kernel holds in registers; anything else takes the synchronous loop"""
    from .architecture import DetectionLoss
    return bool(getattr(opt, "async_eval", False)) and type(criterion) is DetectionLoss and \
        2 <= int(getattr(model, "n_classes", 0)) <= 32


def _device_metrics_apply(model, criterion, opt, steps):
    """opt.device_metrics takes effect where the asynchronous evaluation does and a slot's mask holds the thresholds"""
    return bool(getattr(opt, "device_metrics", False)) and _async_eval_applies(model, criterion, opt) and \
        1 <= steps <= ops.METRICS_MAX_THRESHOLDS


def _eval_streams(opt):
    n = getattr(opt, "eval_streams", None)
    if n is None:
        return None
    if isinstance(n, int):
        return [torch.cuda.Stream() for _ in range(n)]
    return list(n)


def test(model, test_loader, criterion, opt):
    """train.py:324-508.  Returns the mean AP at the last IoU threshold (None when nothing was detected), like the
    reference; the per-threshold mAPs, MAP@ALL, top-1 accuracy and mean losses are left in ``opt.test_report``.
    ``opt.async_eval`` (absent: the loop below as it always was): the batches go through ``evaluate_stream`` with
    ``opt.eval_depth`` (default 4) in flight on ``opt.eval_streams`` streams (a count or a list; default the current
    stream) when the criterion is DetectionLoss — same value, same report, plus ``report["confusion"]``, the [K, K]
    counts summed over the batches.
    ``opt.device_metrics`` (off by default; only where ``opt.async_eval`` applies and ``map_step <= 32``): no handle is
    read, the epoch is accumulated on the device (``EpochMetrics``, ``opt.metrics_capacity`` images to start with) and AP
    per class and threshold is computed there — one device -> host copy per epoch; the same keys in the report.  Equal
    scores keep epoch order there, where numpy's argsort leaves their order open."""
    model.eval()
    steps = int(getattr(opt, "map_step", 10))
    ths = np.linspace(0.5, 0.95, steps)
    metrics, labels, losses = [[] for _ in range(steps)], [], {}
    n_true = n_total = 0
    confusion = None
    classifier = getattr(opt, "classifier", "softmax")
    with torch.no_grad():
        acc = None
        if _device_metrics_apply(model, criterion, opt, steps):
            acc = EpochMetrics(model, ths, capacity_images=int(getattr(opt, "metrics_capacity", 1024)))
        if acc is not None or _async_eval_applies(model, criterion, opt):
            reps = evaluate_stream(model, test_loader, depth=int(getattr(opt, "eval_depth", 4)), streams=_eval_streams(opt),
                                   metrics=acc, fixup=True, classifier=classifier, iou_thresholds=ths)
        else:
            reps = (evaluate_batch(model, criterion, data, slices, classifier=classifier, iou_thresholds=ths,
                                   device_post=bool(getattr(opt, "device_postprocess", False)))
                    for data, slices in test_loader)
        if acc is not None:
            for _ in reps:
                pass
            rep = acc.result()
            if rep is None:
                return None
            opt.test_report = {k: rep[k] for k in ("iou_thresholds", "map", "top1", "loss", "confusion", "map_all")}
            opt.test_value = rep["map"][-1]
            return opt.test_value
        for rep in reps:
            for t in range(steps):
                metrics[t] += rep["sample_metrics"][t]
            labels += rep["labels"]
            n_true, n_total = n_true + rep["n_true"], n_total + rep["n_total"]
            for k, v in rep["loss"].items():
                losses.setdefault(k, []).append(v)
            if "confusion" in rep:
                confusion = rep["confusion"].copy() if confusion is None else confusion + rep["confusion"]
    report = {"iou_thresholds": ths, "map": [], "top1": n_true / max(n_total, 1),
              "loss": {k: float(np.mean(v)) for k, v in losses.items()}}
    if confusion is not None:
        report["confusion"] = confusion
    ap = None
    for t in range(steps):
        if len(metrics[t]) == 0:
            return None
        tp, scores, plabels = [np.concatenate([np.asarray(a) for a in col], 0) for col in zip(*metrics[t])]
        _, _, ap, _, _ = ap_per_class(tp, scores, plabels, np.asarray(labels))
        report["map"].append(float(np.mean(ap)) if len(ap) else 0.0)
    report["map_all"] = float(np.sum(report["map"]) / 10)             # the reference divides by 10 (train.py:484)
    opt.test_report = report
    opt.test_value = float(np.mean(ap)) if ap is not None and len(ap) else 0.0
    return opt.test_value
