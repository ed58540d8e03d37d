"""CPU tests (-m "not gpu") of the batched detection post-processing entry points (csrc/detect.hip): argument
validation before any launch, the work-space query, and the Python surface refusing what it cannot run."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib


def test_new_entry_points_are_declared_on_both_sides():
    for name in ("yolat_detect_scores", "yolat_nms_batched_work_bytes", "yolat_nms_batched", "yolat_detect_match"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    for name in ("non_max_suppression_batched", "get_batch_statistics_batched", "detect_batch"):
        assert callable(getattr(yv, name))
    for name in ("detect_scores", "nms_batched", "detect_match"):
        assert callable(getattr(yv.ops, name))


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = _lib.lib
    one = 4096          # any non-null address: validation never dereferences
    # scores: null pointers, negative sizes, K < 2, ld < K
    assert lib.yolat_detect_scores(None, 5, 3, 3, None, None, 1, None, 1, None, None) == -1
    assert lib.yolat_detect_scores(one, -1, 3, 3, one, one, 1, one, 1, one, None) == -1
    assert lib.yolat_detect_scores(one, 5, 1, 1, one, one, 1, one, 1, one, None) == -1
    assert lib.yolat_detect_scores(one, 5, 3, 2, one, one, 1, one, 1, one, None) == -1
    assert lib.yolat_detect_scores(one, 5, 3, 3, one, one, 0, one, 1, one, None) == -1
    assert lib.yolat_detect_scores(one, 5, 3, 3, one, one, 1, one, 1, None, None) == -1
    # batched nms
    assert lib.yolat_nms_batched(None, 5, 3, None, 1, 0.1, 0.5, 0, None, None, None, 0, None) == -1
    assert lib.yolat_nms_batched(one, -1, 3, one, 1, 0.1, 0.5, 0, one, one, one, 1 << 20, None) == -1
    assert lib.yolat_nms_batched(one, 5, 0, one, 1, 0.1, 0.5, 0, one, one, one, 1 << 20, None) == -1
    assert lib.yolat_nms_batched(one, 5, 3, one, 0, 0.1, 0.5, 0, one, one, one, 1 << 20, None) == -1
    assert lib.yolat_nms_batched(None, 5, 3, one, 1, 0.1, 0.5, 0, one, one, one, 1 << 20, None) == -1
    assert lib.yolat_nms_batched(one, 5, 3, one, 1, 0.1, 0.5, 0, one, one, one, 0, None) == -1       # work too small
    assert lib.yolat_nms_batched(one, 5, 5000, one, 1, 0.1, 0.5, 0, one, one, one, 1 << 20, None) == -2
    assert lib.yolat_nms_batched(one, 5, 3, one, 1, 0.1, 0.5, 0, one, one, one + 8, 1 << 20, None) == -2   # alignment
    # match
    assert lib.yolat_detect_match(None, None, 1, None, None, 0, None, None, 1, None, None) == -1
    assert lib.yolat_detect_match(one, one, 0, one, one, 1, one, one, 1, one, None) == -1
    assert lib.yolat_detect_match(one, one, 1, one, one, -1, one, one, 1, one, None) == -1
    assert lib.yolat_detect_match(one, one, 1, one, one, 1, one, one, 0, one, None) == -1
    assert lib.yolat_detect_match(one, one, 1, None, one, 1, one, one, 1, one, None) == -1
    assert lib.yolat_detect_match(one, one, 1, one, one, 1 << 20, one, one, 1, one, None) == -2
    with pytest.raises(_lib.YolatLibraryError):
        _lib.check(-1, "yolat_nms_batched")


def test_work_bytes_query_is_monotone_linear_and_zero_when_unsupported():
    q = _lib.lib.yolat_nms_batched_work_bytes
    last = 0
    for R in (0, 1, 2, 63, 64, 65, 1000, 2000, 16000, 30000, 100000):
        need = q(R, 16, 8)
        assert need >= last and need > 0
        assert need <= 64 * R * 16 + 65536 * 8            # linear in the candidates: no n x n mask
        last = need
    assert q(2000, 1, 1) <= q(2000, 2, 1) <= q(2000, 17, 1)
    assert q(2000, 16, 1) <= q(2000, 16, 8) + 4096
    for bad in ((-1, 16, 1), (10, 0, 1), (10, 16, 0), (10, 4097, 1), (10, 16, 65537), (1 << 27, 2, 1)):
        assert q(*bad) == 0
    assert yv.ops.nms_batched_work_bytes(2000, 16, 8) == q(2000, 16, 8)


def test_wrappers_refuse_cpu_tensors():
    ptr = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.detect_scores(torch.zeros(4, 3), torch.zeros(4, 4), ptr, torch.ones(1, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.nms_batched(torch.zeros(4, 8), ptr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.detect_match(torch.zeros(1, 300, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(2, 4), torch.zeros(2),
                            torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0.5]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.non_max_suppression_batched(torch.zeros(4, 8), [0, 4])


def test_offsets_are_checked_on_the_host():
    with pytest.raises(ValueError, match="non-decreasing"):
        yv.non_max_suppression_batched(torch.zeros(4, 8), [0, 3, 2, 4])
    with pytest.raises(ValueError, match="non-decreasing"):
        yv.non_max_suppression_batched(torch.zeros(4, 8), [1, 4])
    with pytest.raises(ValueError, match="rows"):
        yv.non_max_suppression_batched(torch.zeros(4, 8), [0, 3])


def test_public_signatures():
    p = inspect.signature(yv.evaluate_batch).parameters
    assert "device_post" in p and p["device_post"].default is False           # the default path stays the per-image one
    p = inspect.signature(yv.non_max_suppression_batched).parameters
    assert list(p) == ["pred_rows", "image_ptr", "conf_thres", "iou_thres", "agnostic"]
    assert (p["conf_thres"].default, p["iou_thres"].default, p["agnostic"].default) == (0.25, 0.45, False)
    assert "classes" not in p and "labels" not in p
    assert "per-image" in yv.non_max_suppression_batched.__doc__
    assert list(inspect.signature(yv.get_batch_statistics_batched).parameters) == ["det", "det_count", "targets", "gt_ptr",
                                                                                  "iou_thresholds"]
    assert list(inspect.signature(yv.detect_batch).parameters)[:5] == ["model", "data", "slices", "conf_thres", "iou_thres"]
    # thresholds travel as fp32: torch compares an fp32 IoU with a threshold rounded to fp32
    assert bool(torch.tensor([0.7], dtype=torch.float32) >= 0.7) and float(np.float32(0.7)) < 0.7
