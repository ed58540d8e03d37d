"""CPU tests (-m "not gpu") of the asynchronous evaluation (csrc/evaluate.hip: yolat_evaluate, yolat_eval_rows;
SparseCADGCN.evaluate_submit, evaluation.evaluate_batch_async / evaluate_stream / confusion_counts): the entry points exist
on both sides of the ABI, the workspace query declines what the rows kernel or the stages around it decline and never
shrinks, every argument check comes in front of the first launch, and the stream driver checks its arguments before
anything runs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_on_both_sides():
    header = open(os.path.join(REPO, "include", "yolat_hip.h")).read()
    for name in ("yolat_evaluate", "yolat_evaluate_workspace_bytes", "yolat_eval_rows"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.lib.yolat_abi_version() == 6                      # entry points are added, the ABI version stays
    for name in ("evaluate_batch_async", "evaluate_stream", "confusion_counts", "EvalHandle"):
        assert hasattr(yv, name)
    assert callable(yv.ops.eval_rows) and callable(yv.EvalHandle.ready) and callable(yv.EvalHandle.result)


def test_signatures_and_defaults():
    p = inspect.signature(yv.SparseCADGCN.evaluate_submit).parameters
    assert list(p) == ["self", "data", "slices", "iou_thresholds", "conf_thres", "iou_thres", "classifier"]
    assert (p["iou_thresholds"].default, p["conf_thres"].default, p["iou_thres"].default, p["classifier"].default) == \
        (None, 0.0, 0.5, None)
    p = inspect.signature(yv.evaluate_stream).parameters
    assert list(p)[:4] == ["model", "batches", "depth", "streams"] and p["depth"].default == 4 and p["streams"].default is None
    assert list(p)[4:] == ["kw"] and p["kw"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(yv.evaluate_batch_async).parameters
    assert list(p) == ["model", "data", "slices", "fixup", "kw"] and p["fixup"].default is True


def test_workspace_query_is_zero_when_unsupported_and_non_decreasing():
    q = _lib.lib.yolat_evaluate_workspace_bytes        # (N, P, R, Ctot, K, B, G, T)
    base = q(10000, 400, 100, 300, 17, 4, 50, 10)
    assert base > 0 and base % 256 == 0
    # yolat_detect's workspace and the per-workgroup partial sums of the loss behind it
    assert base >= _lib.lib.yolat_detect_workspace_bytes(10000, 400, 100, 300, 17, 4) + 4 * ((400 + 255) // 256 + 1)
    for bad in ((10000, 400, 100, 300, 1, 4, 50, 10),            # K = 1
                (10000, 400, 100, 300, 33, 4, 50, 10),           # K = 33: beyond the register-resident row
                (10000, 400, 100, 300, 17, 4, 262145, 10),       # G > 262 144
                (10000, 400, 100, 300, 17, 4, 50, 65536),        # T > 65 535
                (10000, 400, 100, 300, 17, 4, 50, 0), (10000, 400, 100, 300, 17, 4, -1, 10),
                (10000, 400, 100, 300, 17, 0, 50, 10), (10000, 400, 100, 300, 17, 65537, 50, 10),
                (0, 400, 100, 300, 17, 4, 50, 10), (10000, 0, 100, 300, 17, 4, 50, 10),
                (10000, 400, -1, 300, 17, 4, 50, 10), (10000, 400, 1 << 29, 1 << 29, 17, 4, 50, 10)):
        assert q(*bad) == 0, bad
    for K in (2, 32):
        assert q(10000, 400, 100, 300, K, 4, 50, 10) > 0
    assert q(10000, 400, 100, 300, 17, 4, 262144, 65535) > 0 and q(10000, 400, 100, 300, 17, 4, 0, 1) > 0
    for pos, values in ((2, (0, 1, 63, 255, 256, 257, 1000, 5000, 100000)), (3, (0, 1, 255, 256, 257, 1000, 5000, 100000)),
                        (6, (0, 1, 31, 32, 33, 1000, 262144)), (7, (1, 2, 10, 64, 65, 65535))):
        last = 0
        for v in values:
            args = [10000, 400, 100, 300, 17, 4, 50, 10]
            args[pos] = v
            need = q(*args)
            assert need >= last and need > 0, (pos, v)
            last = need
    assert yv.ops.evaluate_workspace_bytes(10000, 400, 100, 300, 17, 4, 50, 10) == base


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = _lib.lib
    one_ = 4096         # any non-null address: validation never dereferences
    al = 1 << 20        # ... and a 256-byte aligned one for the workspace
    t = _lib.PredictTree()
    t.R, t.Ctot, t.B = 3, 2, 1
    for k in ("root_row", "root_range", "child_ptr", "child_row", "child_range", "image_root_ptr"):
        setattr(t, k, one_)
    tp = ctypes.byref(t)

    def call(logits=one_, ld=3, P=5, K=3, bbox=one_, edge=one_, bidx=one_, N=10, E=4, tree=tp, scale=one_, labels=one_,
             gbox=one_, glab=one_, G=2, gptr=one_, ths=one_, T=3, sel=one_, pred=one_, det=one_, cnt=one_, stats=one_,
             loss=one_, ypred=one_, ytrue=one_, tpo=one_, ws=al, wsb=1 << 30):
        return lib.yolat_evaluate(logits, ld, P, K, bbox, edge, 2, 1, bidx, N, E, tree, scale, 1, 0.0, 0.5, labels, gbox,
                                  glab, G, gptr, ths, T, sel, pred, det, cnt, stats, loss, ypred, ytrue, tpo, ws, wsb, None)

    for kw in (dict(logits=None), dict(bbox=None), dict(bidx=None), dict(tree=None), dict(scale=None), dict(labels=None),
               dict(gbox=None), dict(glab=None), dict(gptr=None), dict(ths=None), dict(sel=None), dict(pred=None),
               dict(det=None), dict(cnt=None), dict(stats=None), dict(loss=None), dict(ypred=None), dict(ytrue=None),
               dict(tpo=None), dict(ws=None), dict(edge=None), dict(P=0), dict(K=1), dict(N=0), dict(E=-1), dict(ld=2),
               dict(G=-1), dict(T=0), dict(wsb=64)):
        assert call(**kw) == -1, kw
    assert call(ws=al + 8) == -2                         # alignment
    assert call(K=33, ld=33) == -2                       # beyond the register-resident row
    assert call(G=262145) == -2 and call(T=65536) == -2
    t.B = 0
    assert call() == -1
    t.B, t.R, t.Ctot = 1, 1 << 29, 1 << 29
    assert call() == -2
    # the rows stage alone: (logits, ld, P, K, labels, sel, B, R_cap, softmax, stats, loss, y_pred, y_true, work, stream)
    rows = lib.yolat_eval_rows
    assert rows(None, 3, 5, 3, one_, one_, 1, 4, 1, one_, one_, one_, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, None, one_, 1, 4, 1, one_, one_, one_, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, one_, None, 1, 4, 1, one_, one_, one_, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, one_, one_, 1, 4, 1, None, one_, one_, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, one_, one_, 1, 4, 1, one_, None, one_, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, one_, one_, 1, 4, 1, one_, one_, None, one_, one_, None) == -1
    assert rows(one_, 3, 5, 3, one_, one_, 1, 4, 1, one_, one_, one_, one_, None, None) == -1
    assert rows(one_, 3, 5, 1, one_, one_, 1, 4, 1, one_, one_, one_, one_, one_, None) == -1      # K < 2
    assert rows(one_, 2, 5, 3, one_, one_, 1, 4, 1, one_, one_, one_, one_, one_, None) == -1      # ld < K
    assert rows(one_, 3, 5, 3, one_, one_, 0, 4, 1, one_, one_, one_, one_, one_, None) == -1      # B < 1
    assert rows(one_, 3, 5, 3, one_, one_, 1, -1, 1, one_, one_, one_, one_, one_, None) == -1
    assert rows(one_, 33, 5, 33, one_, one_, 1, 4, 1, one_, one_, one_, one_, one_, None) == -2    # K > 32


def test_confusion_counts_on_a_hand_written_case():
    y_true = [0, 1, 1, 2, 2, 2, 3, -1, 1]        # 3 and -1 are outside [0, 3): ignored
    y_pred = [0, 1, 0, 2, 2, 1, 0, 0, 1]
    got = yv.confusion_counts(y_true, y_pred, 3)
    assert got.dtype == np.int64 and got.shape == (3, 3)
    np.testing.assert_array_equal(got, [[1, 0, 0], [1, 2, 0], [0, 1, 2]])      # rows: true class, columns: predicted
    assert int(got.sum()) == 7
    np.testing.assert_array_equal(yv.confusion_counts(np.zeros(0, np.int64), np.zeros(0, np.int64), 2), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        yv.confusion_counts([0, 1], [0], 2)


def test_evaluate_stream_checks_its_arguments_before_anything_runs():
    with pytest.raises(ValueError, match="depth"):
        next(yv.evaluate_stream(None, [], depth=0))
    with pytest.raises(ValueError, match="streams"):
        next(yv.evaluate_stream(None, [], depth=2, streams=[None] * 5))
    with pytest.raises(ValueError, match="streams"):
        next(yv.evaluate_stream(None, [], depth=2, streams=[]))
    assert list(yv.evaluate_stream(None, [], depth=2)) == []


def test_wrappers_refuse_cpu_tensors_and_unsupported_class_counts():
    import torch
    sel = torch.zeros(4 + 2 + 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.eval_rows(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64), sel, 1, 6)
    with pytest.raises(RuntimeError, match="eval"):
        yv.SparseCADGCN(yv.Opt(n_classes=3)).train().evaluate_submit(None, None)


def test_async_eval_is_taken_only_for_detection_loss_and_supported_class_counts():
    from yolat_vectorgraphicsrecognition_amd import evaluation

    class Other(yv.DetectionLoss):
        pass

    class M(object):
        n_classes = 17

    opt = yv.Opt()
    crit = yv.DetectionLoss(opt)
    assert not evaluation._async_eval_applies(M(), crit, opt)          # the attribute is absent: today's loop
    opt.async_eval = True
    assert evaluation._async_eval_applies(M(), crit, opt)
    assert not evaluation._async_eval_applies(M(), Other(opt), opt)    # any other criterion: the synchronous loop
    M.n_classes = 33
    assert not evaluation._async_eval_applies(M(), crit, opt)


def test_evaluation_record_layout_is_the_one_the_kernels_were_given():
    """int32 offsets of the EvalHandle's record at B=2, K=3, T=2, R_cap=5, written out by hand from
    det_count [B] | stats [2 + K K] | loss | y_pred [R_cap] | y_true [R_cap] | det [B 300 6] | tp [T B 300 bytes] | sel"""
    from yolat_vectorgraphicsrecognition_amd import submit
    assert yv.ops.sel_words(2, 5) == 12 and yv.ops.sel_words(1, 0) == 6
    rec = submit.EvalRecord(2, 3, 2, 5)
    assert rec.off == {"det_count": 0, "stats": 2, "loss": 13, "y_pred": 14, "y_true": 19, "det": 24, "tp": 3624, "sel": 3924}
    assert rec.copy == 3928 and rec.words == 3936
    host = np.arange(rec.copy, dtype=np.int32)
    det, det_count, tp, stats, loss = rec.views(host)
    assert det.shape == (2, 300, 6) and det.dtype == np.float32 and det.view(np.int32)[0, 0, 0] == 24
    assert tp.shape == (2, 2, 300) and tp.dtype == np.uint8 and tp[0, 0, :4].tolist() == [0x28, 0x0E, 0, 0]      # word 3624
    assert det_count.tolist() == [0, 1] and stats.tolist() == list(range(2, 13)) and loss.view(np.int32).tolist() == [13]
    total, flag, status, image_off, rows = yv.ops.sel_split(np.arange(12), 2)
    assert (total, flag, status) == (0, 1, 2) and image_off.tolist() == [4, 5, 6] and rows.tolist() == [7, 8, 9, 10, 11]


@pytest.mark.parametrize("depth,want", [
    (2, "s0 s1 r0 s2 r1 s3 r2 s4 r3 r4"), (1, "s0 r0 s1 r1 s2 r2 s3 r3 s4 r4"), (7, "s0 s1 s2 s3 s4 r0 r1 r2 r3 r4")])
def test_in_flight_reads_the_oldest_handle_once_depth_are_flying(depth, want):
    from yolat_vectorgraphicsrecognition_amd import evaluation
    log = []

    class Handle(object):
        def __init__(self, i):
            self.i = i

        def result(self):
            log.append("r%d" % self.i)
            return self.i

    def submitted():
        for i in range(5):
            log.append("s%d" % i)
            yield Handle(i)

    assert list(evaluation._in_flight(submitted(), depth)) == [0, 1, 2, 3, 4]
    assert " ".join(log) == want
