"""The submissions behind ``SparseCADGCN.predict`` / ``detect_submit`` / ``evaluate_submit``: ONE eval forward over the whole
batch, then the integer selection of the reference's two passes on the device (csrc/subgraph.hip) — alone
(``predict_one_submission``, one read at the end), followed by scores and NMS (``detect_submit``, csrc/detect.hip), or by the
whole evaluation iteration (``evaluate_submit``, csrc/evaluate.hip); the last two read nothing and return a handle.

The three share their front half (``_front``), the flattened tree and its one upload (``predict_tree``), the image scales
(``image_scales``) and the ride-along of the forward's status word (``_ride_status``); the handles share ``_Handle``.  The
record of the selection is ``ops.sel_words`` / ``ops.sel_split``'s, the record of an ``EvalHandle`` is ``EvalRecord``."""
import ctypes

import numpy as np
import torch

from . import ops
from ._lib import lib, check, PredictTree
from .data import flatten_tree, collate_to_device

PREPARED_BATCH = ("predict() cuts sub-graphs out of the raw edge list: batches from collate_to_device(csr=True) "
                  "carry the prepared CSR only and support forward() — collate with csr=False for predict()")


def require_raw_edges(data):
    """ValueError for a batch that carries the prepared CSR only (collate_to_device(csr=True)), not its raw edge list"""
    if getattr(data, "_yolat_graph", None) is not None and not all(k in data.keys for k in ("edge", "e_attr", "bbox_idx")):
        raise ValueError(PREPARED_BATCH)


class _Handle(object):
    """What DetectHandle and EvalHandle share: ``sel``, ``pred`` and the workspace, the event behind the last launch, the batch
    retained for the fall-back, and the decision ``result()`` takes from the two flags of the selection's record."""

    def __init__(self, model, data, slices, sel, pred, workspace, event, kw):
        self.model, self.data, self.slices, self.kw = model, data, slices, kw
        self.sel, self.pred, self.workspace, self.event = sel, pred, workspace, event
        self.device = sel.device
        self._result = None

    def ready(self):
        return bool(self.event.query())

    def _release(self):
        self.data = self.slices = self.pred = self.workspace = None

    def _retained_batch(self):
        """(data, slices, fresh): a DeviceLoader batch is collated again from its host items — its ring slot may have been
        rewritten since — and is then the handle's own (fresh)"""
        data = self.data
        st = data.__dict__.get("_lazy") if hasattr(data, "__dict__") else None
        if st is None:
            return data, self.slices, False
        return collate_to_device(st.items, device=self.device) + (True,)

    def _settle(self, status, flag, form):
        """result() behind its one read: a flagged forward raises, a flagged tree falls back, else ``form()`` of the record"""
        if status != 0:
            ops.check_status_word(torch.tensor([status], dtype=torch.int32))      # raises for every flag a forward sets
        self._result = self._fallback() if flag != 0 else form()
        self._release()
        return self._result


class DetectHandle(_Handle):
    """One batch of ``SparseCADGCN.detect_submit`` in flight.  It owns the device tensors of its batch — ``sel`` (the
    record of yolat_predict_select), ``pred`` [R + Ctot, 4 + K], ``det`` [B, 300, 6], ``det_count`` [B] and the workspace —
    allocated on the submitting stream and released with the handle, and keeps the batch for the fall-back.

    ``ready()``   the event behind the batch's last launch has completed (a query, no wait)
    ``result()``  the list of B device tensors [k, 6] ``evaluation.detect_batch`` returns; ONE device -> host read
                  (ops.d2h) of sel[0:4] and the B detection counts.  A forward that flagged its input raises what
                  ``check_last_status`` raises; a tree that is not made of its proposals' ranges (sel[1]) goes through the
                  synchronous ``detect_batch`` on the retained batch — a DeviceLoader batch is collated again from its
                  host items, its ring slot may have been rewritten since."""

    def __init__(self, model, data, slices, out, det, det_count, sel, pred, workspace, event, kw):
        _Handle.__init__(self, model, data, slices, sel, pred, workspace, event, kw)
        self._out, self.det, self.det_count = out, det, det_count

    def result(self):
        if self._result is not None:
            return self._result
        B = int(self.det_count.shape[0])
        n_det = self.det.numel()
        # det_count [B] | the head of sel; stream order: behind the NMS
        host = ops.d2h(self._out[n_det:n_det + B + ops.SEL_HEAD]).tolist()
        _, flag, status, _, _ = ops.sel_split(host[B:], B)
        return self._settle(status, flag, lambda: [self.det[i, :k] for i, k in enumerate(host[:B])])

    def _fallback(self):
        from .evaluation import detect_batch
        data, slices, _ = self._retained_batch()
        return detect_batch(self.model, data, slices, fixup=False, **self.kw)


class EvalRecord(object):
    """The device record of an ``EvalHandle``, ONE int32 allocation ``det_count | stats | loss | y_pred | y_true | det | tp |
    sel``: ``off[name]`` is where a field starts (in int32 words; it ends where the next one starts), ``words`` the whole
    length and ``copy`` what result() reads — sel comes last, so that the copy ends behind sel's head."""
    FIELDS = ("det_count", "stats", "loss", "y_pred", "y_true", "det", "tp", "sel")

    def __init__(self, B, K, T, R_cap):
        self.B, self.K, self.T, self.R_cap = B, K, T, R_cap
        sizes = (B, 2 + K * K, 1, R_cap, R_cap, B * ops.MAX_DET * 6, (T * B * ops.MAX_DET + 3) // 4, ops.sel_words(B, R_cap))
        self.off, o = {}, 0
        for name, n in zip(self.FIELDS, sizes):
            self.off[name] = o
            o += n
        self.words, self.copy = o, self.off["sel"] + ops.SEL_HEAD

    def views(self, buf):
        """(det [B, 300, 6] fp32, det_count [B], tp [T, B, 300] uint8, stats [2 + K * K], loss [1] fp32) of ``buf``: the
        device tensor, or the numpy array of its first ``copy`` words"""
        f32, u8 = (torch.float32, torch.uint8) if torch.is_tensor(buf) else (np.float32, np.uint8)
        B, T, off = self.B, self.T, self.off
        det = buf[off["det"]:off["tp"]].view(f32).reshape(B, ops.MAX_DET, 6)
        tp = buf[off["tp"]:off["sel"]].view(u8)[:T * B * ops.MAX_DET].reshape(T, B, ops.MAX_DET)
        return det, buf[:B], tp, buf[off["stats"]:off["loss"]], buf[off["loss"]:off["y_pred"]].view(f32)


class EvalHandle(_Handle):
    """One batch of ``SparseCADGCN.evaluate_submit`` in flight.  It owns the device record of its batch — ONE allocation
    ``det_count | stats | loss | y_pred | y_true | det | tp | sel`` (``EvalRecord``) plus ``pred`` and the workspace, allocated
    on the submitting stream and released with the handle — and keeps the batch for the fall-back.  The record is per handle,
    not a global accumulator: a batch that takes the fall-back discards its device record.  ``B``, ``K``, ``T``, ``stream``
    and ``device`` say what was submitted and where.

    ``ready()``   the event behind the batch's last launch has completed (a query, no wait)
    ``result()``  the dict ``evaluation.evaluate_batch`` returns (``sample_metrics``, ``labels``, ``loss``, ``n_true``,
                  ``n_total``, ``y_pred``, ``y_true``) plus ``confusion``, np.int64 [K, K] (rows: true class, columns:
                  predicted); ONE device -> host read (ops.d2h, on the submitting stream) of the record up to sel[0:4].
                  A forward that flagged its input raises what ``check_last_status`` raises; a tree that is not made of
                  its proposals' ranges (sel[1]) goes through ``evaluate_batch(device_post=True, fixup=False)`` on a
                  shallow copy of the retained batch — a DeviceLoader batch is collated again from its host items — and
                  ``confusion`` is then counted on the host."""

    def __init__(self, model, data, slices, out, rec, sel, pred, workspace, event, stream, labels, kw):
        _Handle.__init__(self, model, data, slices, sel, pred, workspace, event, kw)
        self._out, self._rec, self._labels, self.stream = out, rec, labels, stream
        self.B, self.K, self.T = rec.B, rec.K, rec.T

    def result(self):
        if self._result is not None:
            return self._result
        rec = self._rec
        with torch.cuda.stream(self.stream):
            host = ops.d2h(self._out[:rec.copy]).numpy()        # stream order: behind the true-positive walk
            total, flag, status = (int(v) for v in ops.sel_split(host[rec.off["sel"]:], rec.B)[:3])
            return self._settle(status, flag, lambda: self._form(host, min(max(total, 0), rec.R_cap)))

    def _form(self, host, total):
        from .postprocess import _unpack_statistics
        det, det_count, tp, stats, loss = self._rec.views(host)
        K, off = self.K, self._rec.off
        loss = float(loss[0])
        return {"loss": {"loss": loss, "loss_cls": loss}, "n_true": int(stats[0]), "n_total": int(stats[1]),
                "y_pred": host[off["y_pred"]:off["y_pred"] + total].astype(np.int64),
                "y_true": host[off["y_true"]:off["y_true"] + total].astype(np.int64),
                "sample_metrics": _unpack_statistics(det_count, det, tp), "labels": list(self._labels),
                "confusion": stats[2:].reshape(K, K).astype(np.int64)}

    def device_record(self):
        """Views of the device record, nothing read: (det [B, 300, 6], det_count [B], tp [T, B, 300] uint8,
        stats [2 + K * K] int32, loss [1]) — what yolat_metrics_append takes (evaluation.EpochMetrics)"""
        return self._rec.views(self._out)

    def _fallback(self):
        from .architecture import DetectionLoss, Opt
        from .evaluation import evaluate_batch, confusion_counts
        data, slices, fresh = self._retained_batch()
        if not fresh:
            # evaluate_batch overwrites data.labels and slices["bbox"], as the reference does: not on the caller's objects
            bag = data.__class__()
            bag.__dict__.update(data.__dict__)
            data, slices = bag, dict(slices)
        kw = self.kw
        crit = DetectionLoss(Opt(classifier=kw["classifier"]))
        with torch.no_grad():
            res = evaluate_batch(self.model, crit, data, slices, classifier=kw["classifier"],
                                 iou_thresholds=kw["iou_thresholds"], conf_thres=kw["conf_thres"],
                                 iou_thres=kw["iou_thres"], fixup=False, device_post=True)
        res["confusion"] = confusion_counts(res["y_true"], res["y_pred"], self.K)
        return res


def predict_operands(model, data, logits, bbox):
    """(edge address, its two strides, bbox_idx address, N, E, P, device) of the batch whose forward just ran — what
    yolat_predict_select validates the tree against; None when the edge list is not [E, 2]"""
    d = data.__dict__ if hasattr(data, "__dict__") else {}
    raw = d.get("_yolat_raw")
    if raw is not None:
        _, _, ep, se, sc, _, bp, N, E, P, dev = raw
        return ep, se, sc, bp, N, E, P, dev
    st = model._stage_tensors(data)
    edge, bidx = st["edge"], st["bbox_idx"]
    if edge.dim() != 2 or edge.shape[1] != 2:
        return None
    return (ops._i(edge, torch.int64, "edge"), edge.stride(0), edge.stride(1), ops._i(bidx, torch.int64, "bbox_idx"),
            st["x"].shape[0], edge.shape[0], bbox.shape[0], logits.device)


def predict_tree(data, slices, dev, scales=None, extra=None):
    """The flattened tree (data.flatten_tree) on the device, uploaded once per batch object (keyed by the identity of
    the tree and the image offsets) -> (yolat_predict_tree, the host arrays, address of the scales or None).
    scales [B, 4] fp32 (detect_submit) travel in the same upload and are cached with it; so do the arrays of
    ``extra`` (evaluate_submit: a list of (name, contiguous numpy array of 4- or 8-byte elements), each placed at an
    8-byte aligned offset) — their device addresses are left in ``tree._addr[name]``.  An upload made under another
    stream is waited for on the current one before it is handed out."""
    d = data.__dict__ if hasattr(data, "__dict__") else {}
    key = (id(data.roots), len(data.roots), tuple(int(v) for v in slices["roots"]), tuple(int(v) for v in slices["pos"]),
           tuple(int(v) for v in slices["edge"]), tuple(int(v) for v in slices["bbox"]))
    ent = d.get("_yolat_tree")
    skey = None if scales is None else scales.tobytes()
    if extra:
        skey = (skey,) + tuple((name, a.dtype.str, a.tobytes()) for name, a in extra)
    if ent is None or ent[0] != key or (skey is not None and ent[4] != skey):
        ft = flatten_tree(data, slices)
        order = ("root_row", "root_range", "child_ptr", "child_row", "child_range", "image_root_ptr")
        parts = [ft[k].reshape(-1) for k in order]
        offs, o = {}, 0
        for k in order:
            offs[k] = o
            o += ft[k].size
        offs["scale"] = o
        if scales is not None:
            parts.append(np.ascontiguousarray(scales, dtype=np.float32).reshape(-1).view(np.int32))
            o += parts[-1].size
        for name, a in (extra or ()):
            if o % 2:
                parts.append(np.zeros(1, dtype=np.int32))
                o += 1
            offs[name] = o
            parts.append(np.ascontiguousarray(a).reshape(-1).view(np.int32))
            o += parts[-1].size
        host = torch.from_numpy(np.concatenate(parts))
        if skey is not None:
            host = host.pin_memory()                 # a copy from pageable memory waits for the stream: predict reads
            #                                          the device next anyway, detect_submit must not wait
        buf = host.to(dev, non_blocking=True)
        buf._yolat_host = host                       # alive until the copy has run: as long as its target
        if extra:
            up = torch.cuda.Event()
            up.record(ops.current_stream_object())
            buf._yolat_upload = (ops._stream(), up)
        ent = (key, ft, buf, offs, skey)
        try:
            data.__dict__["_yolat_tree"] = ent
        except AttributeError:
            pass
    _, ft, buf, offs, have = ent
    upload = getattr(buf, "_yolat_upload", None)
    if upload is not None and upload[0] != ops._stream():
        cur = ops.current_stream_object()
        cur.wait_event(upload[1])
        buf.record_stream(cur)
    t = PredictTree()
    t.R, t.Ctot, t.B = ft["R"], ft["Ctot"], ft["B"]
    base = buf.data_ptr()
    for k in ("root_row", "root_range", "child_ptr", "child_row", "child_range", "image_root_ptr"):
        setattr(t, k, base + 4 * offs[k])
    t._keep = buf
    t._addr = {name: base + 4 * offs[name] for name, _ in (extra or ())}
    return t, ft, (base + 4 * offs["scale"]) if have is not None else None


def image_scales(data, B):
    """np.float32 [B, 4]: (w, h, w, h) of every image — the pixels the model's unit-square boxes are scaled to — or ones
    for a batch without ``width`` / ``height``"""
    scales = np.ones((B, 4), dtype=np.float32)
    if hasattr(data, "width") and hasattr(data, "height"):
        for i in range(B):
            scales[i] = (float(data.width[i]), float(data.height[i])) * 2
    return scales


def _front(model, data, slices, who=None):
    """The front half of every submission: the no-grad forward of a batch that carries its raw edge list -> (logits, bbox —
    both fp32, rows contiguous —, head, graph, B, dev); ``head`` = (logits address, its row stride, P, K) and ``graph`` =
    (edge address or None, its two strides, bbox_idx address, N, E) are the argument runs around ``bbox`` in the native calls.
    A prepared-CSR batch (no raw edge list to validate the tree against) or an edge list that is not [E, 2]: ``predict``
    (who=None) gets None and goes on to the two-pass extraction, ``who``_submit raises ValueError."""
    d = data.__dict__ if hasattr(data, "__dict__") else {}
    if who is None and d.get("_yolat_graph") is not None:
        return None
    require_raw_edges(data)
    with torch.no_grad():
        logits, bbox = model.forward(data, slices)
    opnd = predict_operands(model, data, logits, bbox)
    if opnd is None:
        if who is None:
            return None
        raise ValueError("%s_submit expects the edge list as [E, 2]" % who)
    ep, se, sc, bp, N, E, P, dev = opnd
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        logits = logits.float().contiguous()
    bb = bbox if (bbox.dtype == torch.float32 and bbox.is_contiguous()) else bbox.float().contiguous()
    head = (logits.data_ptr(), logits.stride(0), P, int(logits.shape[1]))
    return logits, bb, head, (ep if E > 0 else None, se, sc, bp, N, E), len(slices["roots"]) - 1, dev


def _ride_status(model, sel, clear):
    """The input-validity word of the forward that just ran rides along in the record's status word (a device copy in
    stream order).  A submission returns before anyone can look at it, so it clears the forward's word behind the copy and
    the next handle carries the flags of ITS forward only; predict reads the record in the same call and lets
    ``check_last_status()`` raise from the forward's word, which therefore has to stay as it is."""
    status = getattr(model.__dict__.get("_yolat_plan"), "_status", None)
    if status is not None:
        sel[ops.SEL_STATUS:ops.SEL_STATUS + 1].copy_(status)
        if clear:
            status.zero_()


def _done_event():      # -> (an event behind everything enqueued so far on the current stream, that stream)
    cur = ops.current_stream_object()
    done = torch.cuda.Event()
    done.record(cur)
    return done, cur


def predict_one_submission(model, data, slices):
    """One forward over the whole batch, then yolat_predict_select / yolat_predict_gather (csrc/subgraph.hip): in eval
    mode the logits of a proposal depend only on its own nodes and edges, so the root pass and the child pass of the
    reference are rows of the same forward; `has_object` (:259-281), the per-image interleaving (:317-328) and the 5 %
    box enlargement (:341-346) are device kernels.  Returns None when the shortcut does not apply (the device found
    tree ranges that are not the ranges of the proposals, or an edge between proposals: the duplicate / KeyError
    cases of the reference) — the caller then runs the two-pass extraction."""
    front = _front(model, data, slices)
    if front is None:
        return None
    logits, bb, head, graph, _, dev = front
    t, ft, _ = predict_tree(data, slices, dev)
    B, K = ft["B"], head[3]
    out = torch.empty(ops.sel_words(B, ft["R"] + ft["Ctot"]), dtype=torch.int32, device=dev)
    need = int(lib.yolat_predict_select_workspace_bytes(graph[4], head[2], ft["R"])) + 16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = ops._stream()
    check(lib.yolat_predict_select(*head, *graph, ctypes.byref(t), out.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "yolat_predict_select")
    _ride_status(model, out, clear=False)
    total, flag, status, image_off, rows = ops.sel_split(out.cpu().numpy(), B)      # the ONE host read (synchronises)
    if int(status) != 0:
        model.check_last_status()                     # raises IndexError / ValueError like the forward's own check
    if int(flag) != 0:
        return None
    total = int(total)
    pred_cls = torch.empty(total, K, dtype=torch.float32, device=dev)
    pred_bbox = torch.empty(total, 4, dtype=torch.float32, device=dev)
    check(lib.yolat_predict_gather(*head, bb.data_ptr(), out.data_ptr() + 4 * ops.sel_words(B, 0), total, pred_cls.data_ptr(),
                                   pred_bbox.data_ptr(), stream), "yolat_predict_gather")      # (rows: behind B + 1 offsets)
    pred_cls._yolat_keep = (out, logits, bb)
    return pred_cls, pred_bbox, None, torch.from_numpy(rows[:total].astype(np.int64)), [int(v) for v in image_off], None


def detect_submit(model, data, slices, conf_thres, iou_thres, agnostic, classifier):
    if model.training:
        raise RuntimeError("detect_submit runs the eval forward: call model.eval() first")
    logits, bb, head, graph, B, dev = _front(model, data, slices, "detect")
    t, ft, scale_ptr = predict_tree(data, slices, dev, image_scales(data, B))
    R_cap, K = ft["R"] + ft["Ctot"], head[3]
    need = int(lib.yolat_detect_workspace_bytes(graph[4], head[2], ft["R"], ft["Ctot"], K, B))
    if need == 0:
        raise ValueError("detect_submit: a batch of %d images, %d tree nodes and %d classes is outside what the batched "
                         "NMS supports (nc <= 4096, B <= 65536, rows * nc <= 2^27)" % (B, R_cap, K))
    # one allocation for what result() looks at and what it returns: det [B, 300, 6] | det_count [B] | sel
    n_det = B * ops.MAX_DET * 6
    out = torch.empty(n_det + B + ops.sel_words(B, R_cap), dtype=torch.int32, device=dev)
    det, det_count, sel = out[:n_det].view(torch.float32).view(B, ops.MAX_DET, 6), out[n_det:n_det + B], out[n_det + B:]
    pred = torch.empty((R_cap, 4 + K), dtype=torch.float32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    cls = model.classifier if classifier is None else classifier
    check(lib.yolat_detect(*head, bb.data_ptr(), *graph, ctypes.byref(t), scale_ptr, int(cls == "softmax"),
                           float(conf_thres), float(iou_thres), int(bool(agnostic)), sel.data_ptr(), pred.data_ptr(),
                           det.data_ptr(), det_count.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "yolat_detect")
    _ride_status(model, sel, clear=True)
    return DetectHandle(model, data, slices, out, det, det_count, sel, pred, ws, _done_event()[0],
                        dict(conf_thres=conf_thres, iou_thres=iou_thres, agnostic=agnostic, classifier=cls))


def evaluate_submit(model, data, slices, iou_thresholds, conf_thres, iou_thres, classifier):
    if model.training:
        raise RuntimeError("evaluate_submit runs the eval forward: call model.eval() first")
    require_raw_edges(data)                              # in front of the label check, which is in front of the forward
    if iou_thresholds is None:
        iou_thresholds = np.linspace(0.5, 0.95, 10)
    ths = np.ascontiguousarray(np.asarray(iou_thresholds, dtype=np.float32).reshape(-1))
    labels = data.labels
    if not labels.is_cuda and labels.numel():
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= model.n_classes:
            raise IndexError("Target %d is out of bounds." % (lo if lo < 0 else hi))
    logits, bb, head, graph, B, dev = _front(model, data, slices, "evaluate")
    P, K, T = head[2], head[3], int(ths.shape[0])
    scales = image_scales(data, B)
    # the targets of evaluate_batch: rows label_ptr[i]:label_ptr[i + 1] of image i, boxes scaled in fp32
    lptr = np.asarray([int(v) for v in slices["gt_labels"]], dtype=np.int64)
    if lptr.shape[0] != B + 1:
        raise ValueError("slices['gt_labels'] must hold B + 1 offsets")
    g0, g1 = int(lptr[0]), int(lptr[-1])
    per_image = np.repeat(np.arange(B), np.diff(lptr))
    gt_labels = data.gt_labels[g0:g1].cpu()
    gt_box = (data.gt_bbox[g0:g1].cpu().float() * torch.from_numpy(scales)[torch.from_numpy(per_image)]).numpy()
    G = int(gt_box.shape[0])
    extra = [("gt_ptr", (lptr - g0).astype(np.int32)), ("gt_box", np.ascontiguousarray(gt_box, dtype=np.float32)),
             ("gt_label", gt_labels.float().numpy()), ("thresholds", ths)]
    if not labels.is_cuda:
        extra.append(("labels", np.ascontiguousarray(labels.numpy(), dtype=np.int64)))
    elif labels.dtype != torch.int64 or not labels.is_contiguous():
        labels = labels.long().contiguous()
    if int(labels.shape[0]) != P:
        raise ValueError("labels must hold one class id per proposal")
    t, ft, scale_ptr = predict_tree(data, slices, dev, scales, extra)
    R_cap = ft["R"] + ft["Ctot"]
    need = int(lib.yolat_evaluate_workspace_bytes(graph[4], P, ft["R"], ft["Ctot"], K, B, G, T))
    if need == 0:
        raise ValueError("evaluate_submit: a batch of %d images, %d tree nodes, %d classes, %d targets and %d thresholds "
                         "is outside what yolat_evaluate supports (K in [2, 32], B <= 65536, rows * (K - 1) <= 2^27, "
                         "targets <= 262144, thresholds <= 65535)" % (B, R_cap, K, G, T))
    rec = EvalRecord(B, K, T, R_cap)
    out = torch.empty(rec.words, dtype=torch.int32, device=dev)
    sel = out[rec.off["sel"]:]
    pred = torch.empty((R_cap, 4 + K), dtype=torch.float32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    cls = model.classifier if classifier is None else classifier
    addr, at = t._addr, {name: out.data_ptr() + 4 * o for name, o in rec.off.items()}
    check(lib.yolat_evaluate(*head, bb.data_ptr(), *graph, ctypes.byref(t), scale_ptr, int(cls == "softmax"),
                             float(conf_thres), float(iou_thres), addr["labels"] if "labels" in addr else labels.data_ptr(),
                             addr["gt_box"], addr["gt_label"], G, addr["gt_ptr"], addr["thresholds"], T, at["sel"],
                             pred.data_ptr(), at["det"], at["det_count"], at["stats"], at["loss"], at["y_pred"],
                             at["y_true"], at["tp"], ws.data_ptr(), ws.numel(), ops._stream()), "yolat_evaluate")
    _ride_status(model, sel, clear=True)
    done, cur = _done_event()
    out._yolat_keep = (logits, bb, labels, t)            # what the launches read: alive as long as the handle's record
    h = EvalHandle(model, data, slices, out, rec, sel, pred, ws, done, cur, gt_labels.tolist(),
                   dict(conf_thres=conf_thres, iou_thres=iou_thres, classifier=cls, iou_thresholds=iou_thresholds))
    # the uploaded target classes [G] fp32, for the epoch record (evaluation.EpochMetrics)
    g_at = (addr["gt_label"] - t._keep.data_ptr()) // 4
    h.gt_label = t._keep[g_at:g_at + G].view(torch.float32)
    return h
