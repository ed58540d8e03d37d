"""The reference's evaluation loop (cad_recognition/train.py:324-508, ``test``) on the device path: per batch the
index fix-up, the two-pass ``model.predict``, the loss, top-1 accuracy, and per image
softmax -> [1 - P(last class), P(other classes)] -> class-aware NMS -> true-positive statistics at the IoU
thresholds 0.5 .. 0.95; then AP per class and threshold.  Same inputs (``(data, slices)`` batches of collated items
with ``labels, has_obj, gt_bbox, gt_labels, width, height`` next to the graph tensors) and the same value written to
``opt.test_value`` / returned (the mean AP at the LAST threshold, train.py:507-508); the intermediate numbers the
reference only logs are returned in ``opt.test_report``."""
import numpy as np
import torch

from .data import fixup_offsets
from . import ops
from .postprocess import (non_max_suppression, get_batch_statistics, ap_per_class, detect_post_device,
                          non_max_suppression_batched)


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
    if fixup:
        fixup_offsets(data, slices)                                   # train.py:346-366
    if not hasattr(data, "edge_control"):
        data.edge_control = None
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
    if fixup:
        fixup_offsets(data, slices)
    if not hasattr(data, "edge_control"):
        data.edge_control = None
    with torch.no_grad():
        out = model.predict(data, slices)
    logits, boxes, image_ptr = out[0].detach().float(), out[1].detach().float().contiguous(), out[4]
    B = len(image_ptr) - 1
    scales = np.ones((B, 4), dtype=np.float32)
    if hasattr(data, "width") and hasattr(data, "height"):
        for i in range(B):
            scales[i] = (float(data.width[i]), float(data.height[i])) * 2
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
    if fixup:
        fixup_offsets(data, slices)
    if not hasattr(data, "edge_control"):
        data.edge_control = None
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
    from collections import deque
    from .data import DeviceLoader
    depth = int(depth)
    if depth < 1:
        raise ValueError("detect_stream needs depth >= 1")
    if isinstance(batches, DeviceLoader):
        slots = getattr(batches, "_slots", None)
        if not isinstance(slots, int):
            raise ValueError("detect_stream cannot tell how many slots the loader has")
        if depth > slots - 2:
            raise ValueError("detect_stream(depth=%d) over a DeviceLoader needs slots >= depth + 2, the loader has %d"
                             % (depth, slots))
    kw.setdefault("fixup", False)
    flying = deque()
    for data, slices in batches:
        flying.append(detect_batch_async(model, data, slices, **kw))
        if len(flying) >= depth:
            yield flying.popleft().result()
    while flying:
        yield flying.popleft().result()


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
    if fixup:
        fixup_offsets(data, slices)
    if not hasattr(data, "edge_control"):
        data.edge_control = None
    return model.evaluate_submit(data, slices, **kw)


MAX_EVAL_STREAMS = 4


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
    belongs to the stream its batches are drawn on (ValueError otherwise)."""
    from collections import deque
    from .data import DeviceLoader
    depth = int(depth)
    if depth < 1:
        raise ValueError("evaluate_stream needs depth >= 1")
    if streams is not None:
        streams = list(streams)
        if not 1 <= len(streams) <= MAX_EVAL_STREAMS:
            raise ValueError("evaluate_stream takes 1 to %d streams, got %d" % (MAX_EVAL_STREAMS, len(streams)))
    if isinstance(batches, DeviceLoader):
        if streams is not None and len(streams) > 1:
            raise ValueError("evaluate_stream over a DeviceLoader takes one stream: the loader's ring belongs to the stream "
                             "its batches are drawn on")
        slots = getattr(batches, "_slots", None)
        if not isinstance(slots, int):
            raise ValueError("evaluate_stream cannot tell how many slots the loader has")
        if depth > slots - 2:
            raise ValueError("evaluate_stream(depth=%d) over a DeviceLoader needs slots >= depth + 2, the loader has %d"
                             % (depth, slots))
    kw.setdefault("fixup", False)
    flying = deque()
    if streams is None:
        for data, slices in batches:
            flying.append(evaluate_batch_async(model, data, slices, **kw))
            if len(flying) >= depth:
                yield flying.popleft().result()
    elif isinstance(batches, DeviceLoader):
        # the draws themselves happen under the stream: the loader hands a slot back behind an event on the drawing stream
        entry = torch.cuda.Event()
        entry.record(ops.current_stream_object())
        streams[0].wait_event(entry)
        it = iter(batches)
        while True:
            with torch.cuda.stream(streams[0]):
                nxt = next(it, None)
                if nxt is None:
                    break
                flying.append(evaluate_batch_async(model, nxt[0], nxt[1], **kw))
            if len(flying) >= depth:
                yield flying.popleft().result()
    else:
        home = ops.current_stream_object()
        entry = torch.cuda.Event()
        entry.record(home)
        for s in streams:
            s.wait_event(entry)
        for i, (data, slices) in enumerate(batches):
            s = streams[i % len(streams)]
            drawn = torch.cuda.Event()
            drawn.record(home)
            s.wait_event(drawn)
            with torch.cuda.stream(s):
                flying.append(evaluate_batch_async(model, data, slices, **kw))
            if len(flying) >= depth:
                yield flying.popleft().result()
    while flying:
        yield flying.popleft().result()


def _async_eval_applies(model, criterion, opt):
    """test() takes evaluate_stream when opt.async_eval is set, the criterion is DetectionLoss itself (what the rows stage
    computes) and the class count is one the rows kernel holds in registers; anything else takes the synchronous loop"""
    from .architecture import DetectionLoss
    return bool(getattr(opt, "async_eval", False)) and type(criterion) is DetectionLoss and \
        2 <= int(getattr(model, "n_classes", 0)) <= 32


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
    counts summed over the batches."""
    model.eval()
    steps = int(getattr(opt, "map_step", 10))
    ths = np.linspace(0.5, 0.95, steps)
    metrics, labels, losses = [[] for _ in range(steps)], [], {}
    n_true = n_total = 0
    confusion = None
    classifier = getattr(opt, "classifier", "softmax")
    with torch.no_grad():
        if _async_eval_applies(model, criterion, opt):
            reps = evaluate_stream(model, test_loader, depth=int(getattr(opt, "eval_depth", 4)), streams=_eval_streams(opt),
                                   fixup=True, classifier=classifier, iou_thresholds=ths)
        else:
            reps = (evaluate_batch(model, criterion, data, slices, classifier=classifier, iou_thresholds=ths,
                                   device_post=bool(getattr(opt, "device_postprocess", False)))
                    for data, slices in test_loader)
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
