"""CPU tests (-m "not gpu") of the asynchronous detection (csrc/detect.hip: yolat_detect, yolat_detect_rows;
SparseCADGCN.detect_submit, evaluation.detect_batch_async / detect_stream): the entry points exist on both sides of the ABI,
the workspace query declines what the batched NMS or yolat_predict_select decline and grows with its arguments, every
argument check comes in front of the first launch, and the rows kernel holds its register budget without scratch."""
import inspect
import os
import re

import pytest

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib

from kernel_meta import CSRC, find_hipcc, kernel_resources, one

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_on_both_sides():
    header = open(os.path.join(REPO, "include", "yolat_hip.h")).read()
    for name in ("yolat_detect", "yolat_detect_workspace_bytes", "yolat_detect_rows"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("detect_batch_async", "detect_stream", "DetectHandle"):
        assert hasattr(yv, name)
    assert callable(yv.SparseCADGCN.detect_submit) and callable(yv.ops.detect_rows) and callable(yv.ops.d2h)
    p = inspect.signature(yv.SparseCADGCN.detect_submit).parameters
    assert list(p) == ["self", "data", "slices", "conf_thres", "iou_thres", "agnostic", "classifier"]
    assert (p["conf_thres"].default, p["iou_thres"].default, p["agnostic"].default, p["classifier"].default) == \
        (0.25, 0.45, False, None)
    assert inspect.signature(yv.detect_stream).parameters["depth"].default == 4
    assert list(inspect.signature(yv.detect_batch_async).parameters) == list(inspect.signature(yv.detect_batch).parameters)


def test_workspace_query_is_zero_when_unsupported_and_non_decreasing():
    q = _lib.lib.yolat_detect_workspace_bytes          # (N, P, R, Ctot, K, B)
    base = q(10000, 400, 100, 300, 17, 4)
    assert base > 0 and base % 256 == 0
    # covers both halves: the selection's workspace and the batched NMS's over R + Ctot rows
    assert base >= _lib.lib.yolat_predict_select_workspace_bytes(10000, 400, 100) + \
        _lib.lib.yolat_nms_batched_work_bytes(400, 16, 4)
    for bad in ((10000, 400, 100, 300, 4098, 4),        # nc = K - 1 > 4096
                (10000, 400, 100, 300, 17, 65537),      # B > 65536
                (10000, 400, 100, 300, 17, 0),          # B < 1
                (10000, 400, 1 << 26, 1 << 26, 3, 4),   # (R + Ctot) * nc > 2^27
                (10000, 400, 100, 300, 1, 4),           # K < 2
                (0, 400, 100, 300, 17, 4), (10000, 0, 100, 300, 17, 4), (10000, 400, -1, 300, 17, 4),
                (10000, 400, 100, -1, 17, 4), (1 << 30, 400, 100, 300, 17, 4)):
        assert q(*bad) == 0, bad
    last = 0
    for R in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 5000, 100000):
        need = q(10000, 400, R, 300, 17, 4)
        assert need >= last > -1 and need > 0
        last = need
    last = 0
    for C in (0, 1, 255, 256, 257, 1000, 5000, 100000):
        need = q(10000, 400, 100, C, 17, 4)
        assert need >= last and need > 0
        last = need
    last = 0
    for K in (2, 3, 4, 17, 32, 33, 100, 1000, 4097):
        need = q(10000, 400, 100, 300, K, 4)
        assert need >= last and need > 0
        last = need
    assert yv.ops.detect_workspace_bytes(10000, 400, 100, 300, 17, 4) == base


def test_invalid_arguments_are_rejected_before_any_launch():
    import ctypes
    lib = _lib.lib
    one_ = 4096         # any non-null address: validation never dereferences
    al = 1 << 20        # ... and a 256-byte aligned one for the workspace
    t = _lib.PredictTree()
    t.R, t.Ctot, t.B = 3, 2, 1
    for k in ("root_row", "root_range", "child_ptr", "child_row", "child_range", "image_root_ptr"):
        setattr(t, k, one_)
    tp = ctypes.byref(t)
    big = 1 << 30

    def call(logits=one_, ld=3, P=5, K=3, bbox=one_, edge=one_, bidx=one_, N=10, E=4, tree=tp, scale=one_, sel=one_,
             pred=one_, det=one_, cnt=one_, ws=al, wsb=big):
        return lib.yolat_detect(logits, ld, P, K, bbox, edge, 2, 1, bidx, N, E, tree, scale, 1, 0.25, 0.45, 0, sel, pred,
                                det, cnt, ws, wsb, None)

    for kw in (dict(logits=None), dict(bbox=None), dict(bidx=None), dict(tree=None), dict(scale=None), dict(sel=None),
               dict(pred=None), dict(det=None), dict(cnt=None), dict(ws=None), dict(edge=None), dict(P=0), dict(K=1),
               dict(N=0), dict(E=-1), dict(ld=2), dict(wsb=64)):
        assert call(**kw) == -1, kw
    assert call(ws=al + 8) == -2                         # alignment
    assert call(K=4098, ld=4098) == -2                   # nc > 4096
    t.B = 0
    assert call() == -1
    t.B, t.R = 1, -1
    assert call() == -1
    t.R, t.Ctot = 1 << 29, 1 << 29
    assert call() == -2
    # the rows kernel alone
    assert lib.yolat_detect_rows(None, 3, 5, 3, one_, one_, 1, 4, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 3, 5, 3, one_, None, 1, 4, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 3, 5, 1, one_, one_, 1, 4, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 2, 5, 3, one_, one_, 1, 4, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 3, 5, 3, one_, one_, 0, 4, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 3, 5, 3, one_, one_, 1, -1, one_, 1, one_, None) == -1
    assert lib.yolat_detect_rows(one_, 3, 5, 3, one_, one_, 1, 0, one_, 1, None, None) == 0      # no rows: nothing to launch
    assert lib.yolat_detect_rows(one_, 5000, 5, 5000, one_, one_, 1, 4, one_, 1, one_, None) == -2


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    sel = torch.zeros(4 + 2 + 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.detect_rows(torch.zeros(5, 3), torch.zeros(5, 4), sel, 1, 6, torch.ones(1, 4))


def test_detect_stream_checks_its_depth_before_anything_runs():
    with pytest.raises(ValueError, match="depth"):
        next(yv.detect_stream(None, [], depth=0))
    assert list(yv.detect_stream(None, [], depth=2)) == []


def test_rows_kernel_holds_its_register_budget_without_scratch():
    """k_detect_rows: one thread per row, a few dozen rows-worth of waves per batch — latency bound, so what matters is that
    nothing spills (a scratch round trip per class) and that the kernel stays as light as the two it fuses
    (k_det_scores 31 VGPRs, k_det_keys 13): at most 64 VGPRs = 8 waves per SIMD, no LDS."""
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    res = kernel_resources(os.path.join(CSRC, "detect.hip"))
    k = one(res, "_ZL13k_detect_rows")
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= 64 and k[".group_segment_fixed_size"] == 0
    # the kernels it rides with keep theirs (pinned nowhere else)
    for prefix, vgpr in (("_ZL12k_det_scores", 64), ("_ZL10k_det_keys", 32), ("_ZL9k_det_nms", 64)):
        kk = one(res, prefix)
        assert kk[".vgpr_spill_count"] == 0 and kk[".private_segment_fixed_size"] == 0 and kk[".vgpr_count"] <= vgpr
