"""CPU tests (-m "not gpu") of the epoch metrics (csrc/metrics.hip, ops.metrics_*, evaluation.EpochMetrics): the entry
points exist and are bound, argument validation and the size queries answer in front of any launch, the wrappers refuse
CPU tensors, the Python surface raises its argument errors, the code objects of the new kernels hold no spill — and
tests/metrics_ref.py, the numpy restatement the GPU tests compare against, equals postprocess.ap_per_class."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

import metrics_ref
import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib
from kernel_meta import CSRC, find_hipcc, kernel_resources

NAMES = ("yolat_metrics_record_bytes", "yolat_metrics_reset", "yolat_metrics_append", "yolat_metrics_append_host",
         "yolat_metrics_finalize_work_bytes", "yolat_metrics_out_bytes", "yolat_metrics_finalize")


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib.yolat_abi_version() == 6


def test_argument_validation_comes_in_front_of_any_launch():
    lib = _lib.lib
    assert lib.yolat_metrics_reset(None, 4, 3, 8, None) == -1
    assert lib.yolat_metrics_append(None, 4, 3, 8, None, None, None, None, None, None, 0, None, 1, 10, 0, 0, None) == -1
    assert lib.yolat_metrics_append_host(None, 4, 3, 8, None, None, None, None, None, None, 0, 1, 10, 0, 0, None) == -1
    assert lib.yolat_metrics_finalize(None, 4, 3, 8, 1, 1, 10, None, 0, None, 0, None) == -1
    # every pointer present (never dereferenced: the calls end in front of the launch) and a bad number
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = (buf.ctypes.data + 255) & ~255
    assert lib.yolat_metrics_append(p, 4, 3, 8, p, p, p, p, p, p, 0, p, 0, 10, 0, 0, None) == -1            # B = 0
    assert lib.yolat_metrics_append(p, 4, 3, 8, p, p, p, p, p, p, 0, p, 2, 10, 3, 0, None) == -1            # image_base + B > cap
    assert lib.yolat_metrics_append(p, 4, 3, 8, p, p, p, p, p, p, 0, p, 1, 10, 0, 8, None) == -1            # batch_index = cap
    assert lib.yolat_metrics_append(p, 4, 3, 8, p, p, p, p, p, p, 0, p, 1, 10, -1, 0, None) == -1
    assert lib.yolat_metrics_append(p, 4, 3, 8, p, p, p, p, p, p, 0, p, 1, 33, 0, 0, None) == -2            # T = 33
    assert lib.yolat_metrics_append(p, 4, 33, 8, p, p, p, p, p, p, 0, p, 1, 10, 0, 0, None) == -2           # K = 33
    assert lib.yolat_metrics_finalize(p, 4, 3, 8, 5, 1, 10, p, 1 << 12, p, 1 << 12, None) == -1            # n_images > cap
    assert lib.yolat_metrics_finalize(p, 4, 3, 8, 1, 1, 33, p, 1 << 12, p, 1 << 12, None) == -2
    assert lib.yolat_metrics_finalize(p, 4, 3, 8, 1, 1, 10, p, 8, p, 1 << 12, None) == -1                  # out too small
    assert lib.yolat_metrics_finalize(p, 4, 3, 8, 1, 1, 10, p, 1 << 12, p, 16, None) == -1                 # work too small
    assert b"invalid" in lib.yolat_strerror(-1)


def test_size_queries_return_zero_outside_the_stated_ranges():
    lib = _lib.lib
    assert lib.yolat_metrics_finalize_work_bytes(1, 10, 3) > 0 and lib.yolat_metrics_finalize_work_bytes(447392, 32, 32) > 0
    for n_images, T, K in ((0, 10, 3), (447393, 10, 3), (1, 0, 3), (1, 33, 3), (1, 10, 1), (1, 10, 33)):
        assert lib.yolat_metrics_finalize_work_bytes(n_images, T, K) == 0, (n_images, T, K)
    assert lib.yolat_metrics_out_bytes(10, 3, 4) == 8 * (3 * 30 + 2 * 3 + 1 + 2 + 9 + 1) + 8 * 4
    for T, K, nb in ((0, 3, 1), (33, 3, 1), (10, 1, 1), (10, 33, 1), (10, 3, 0)):
        assert lib.yolat_metrics_out_bytes(T, K, nb) == 0, (T, K, nb)
    offs = (ctypes.c_int64 * 8)()
    total = lib.yolat_metrics_record_bytes(4, 3, 8, offs)
    S = 4 * 300
    want, o = [], 0
    for n in (4 * S, 4 * S, 4 * S, 8 * 3, 8 * 11, 4 * 8, 8 * 8, 4):
        want.append(o)
        o = (o + n + 255) // 256 * 256
    assert list(offs) == want and total == o
    for cap, K, bcap in ((0, 3, 8), (447393, 3, 8), (4, 1, 8), (4, 33, 8), (4, 3, 0)):
        assert lib.yolat_metrics_record_bytes(cap, K, bcap, None) == 0, (cap, K, bcap)


def test_ops_refuse_cpu_tensors():
    ops = yv.ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.metrics_record(4, 3, 8, "cpu")
    n = int(_lib.lib.yolat_metrics_record_bytes(4, 3, 8, None))
    rec = ops.MetricsRecord(torch.zeros(n, dtype=torch.uint8), 4, 3, 8)
    B, T, K = 2, 10, 3
    det, cnt, tp = torch.zeros(B, 300, 6), torch.zeros(B, dtype=torch.int32), torch.zeros(T, B, 300, dtype=torch.uint8)
    stats, loss, gt = torch.zeros(2 + K * K, dtype=torch.int32), torch.zeros(1), torch.zeros(3)
    sel = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.metrics_append(rec, det, cnt, tp, stats, loss, gt, sel, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.metrics_append_host(rec, det, cnt, tp, stats, loss, gt, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.metrics_finalize(rec, 2, 1, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.metrics_grow(rec, 8, 8)
    with pytest.raises(ValueError, match="outside"):
        ops.MetricsRecord(torch.zeros(n, dtype=torch.uint8), 4, 33, 8)
    with pytest.raises(ValueError, match="at least"):
        ops.MetricsRecord(torch.zeros(n - 1, dtype=torch.uint8), 4, 3, 8)


def test_metrics_unpack_names_the_parts_of_the_block():
    T, K, nb = 2, 3, 2
    words = np.arange(3 * T * K + 2 * K + 1 + 2 + K * K + 1 + nb, dtype=np.int64)
    m = yv.ops.metrics_unpack(words, T, K, nb)
    assert m["ap"].shape == (T, K) and m["ap"].dtype == np.float64
    assert m["ap"].view(np.int64).reshape(-1).tolist() == list(range(6)) and m["r"].view(np.int64)[0, 0] == 12
    assert m["n_gt"].tolist() == [18, 19, 20] and m["n_p"].tolist() == [21, 22, 23]
    assert m["stats"].tolist() == list(range(25, 36)) and m["status"] == 36
    assert m["batch_flags"].shape == (nb, 2) and m["batch_flags"][:, 0].tolist() == [37, 38]


def test_epoch_metrics_and_evaluate_stream_argument_errors():
    model = yv.SparseCADGCN(yv.Opt(n_classes=5))
    assert yv.EpochMetrics(model, np.linspace(0.5, 0.95, 10)).result() is None       # no batch added
    with pytest.raises(ValueError, match="thresholds"):
        yv.EpochMetrics(model, np.linspace(0.5, 0.95, 33))
    with pytest.raises(ValueError, match="thresholds"):
        yv.EpochMetrics(model, [])
    with pytest.raises(ValueError, match="classes"):
        yv.EpochMetrics(yv.SparseCADGCN(yv.Opt(n_classes=33)), [0.5])
    with pytest.raises(ValueError, match="capacity_images"):
        yv.EpochMetrics(model, [0.5], capacity_images=0)
    with pytest.raises(TypeError, match="EvalHandle"):
        yv.EpochMetrics(model, [0.5]).add(object())
    with pytest.raises(TypeError, match="EpochMetrics"):
        next(yv.evaluate_stream(model, [], metrics=object()))
    with pytest.raises(ValueError, match="depth"):
        next(yv.evaluate_stream(model, [], depth=0, metrics=yv.EpochMetrics(model, [0.5])))
    acc = yv.EpochMetrics(model, [0.5])
    assert list(yv.evaluate_stream(model, [], metrics=acc)) == [] and acc.result() is None


def test_device_metrics_switch_is_off_unless_async_eval_applies():
    from yolat_vectorgraphicsrecognition_amd import evaluation as ev
    model = yv.SparseCADGCN(yv.Opt(n_classes=5))
    opt = yv.Opt(n_classes=5)
    crit = yv.DetectionLoss(opt)
    assert not ev._device_metrics_apply(model, crit, opt, 10)
    opt.device_metrics = True
    assert not ev._device_metrics_apply(model, crit, opt, 10)         # without async_eval: today's loop
    opt.async_eval = True
    assert ev._device_metrics_apply(model, crit, opt, 10) and ev._device_metrics_apply(model, crit, opt, 32)
    assert not ev._device_metrics_apply(model, crit, opt, 33)         # a slot's mask holds 32 thresholds

    class Other(yv.DetectionLoss):
        pass
    assert not ev._device_metrics_apply(model, Other(opt), opt, 10)


@pytest.mark.parametrize("seed,K,T,n", [(1, 3, 10, 700), (2, 17, 10, 2500), (3, 2, 1, 50), (4, 32, 32, 4000)])
def test_metrics_ref_equals_ap_per_class_on_tie_free_inputs(seed, K, T, n):
    """threshold by threshold: the reference's arithmetic on the concatenated lists against the record's restatement"""
    rng = np.random.default_rng(seed)
    conf = rng.permutation(n).astype(np.float32) / np.float32(n)          # tie-free
    cls = rng.integers(0, K, size=n).astype(np.float32)
    tp = (rng.random((T, n)) < np.linspace(0.7, 0.1, T)[:, None]).astype(np.uint8)
    gt = rng.integers(0, K, size=max(K, n // 7)).astype(np.float32)
    if K > 2:
        gt[gt == 1] = 0                                                   # a class with detections and no target
        cls[cls == 2] = 0                                                 # a class with targets and no detection
        gt[0] = 2
    rec = metrics_ref.Record(K, T)
    for lo in range(0, n, 300 * 3):                                       # batches of up to three images
        hi = min(n, lo + 900)
        B = (hi - lo + 299) // 300
        det, cnt, tpb = np.zeros((B, 300, 6), np.float32), np.zeros(B, np.int32), np.zeros((T, B, 300), np.uint8)
        for b in range(B):
            a, e = lo + 300 * b, min(hi, lo + 300 * b + 300)
            cnt[b] = e - a
            det[b, :e - a, 4], det[b, :e - a, 5], tpb[:, b, :e - a] = conf[a:e], cls[a:e], tp[:, a:e]
        rec.append(det, cnt, tpb, np.zeros(2 + K * K), 0.0, gt if lo == 0 else [])
    got = rec.finalize()
    assert got["status"] == 0 and int(got["n_p"].sum()) == n and int(got["n_gt"].sum()) == len(gt)
    for t in range(T):
        p, r, ap, f1, classes = yv.ap_per_class(tp[t].astype(np.float64), conf, cls, gt)
        assert classes.tolist() == np.flatnonzero(got["n_gt"] > 0).tolist()
        np.testing.assert_allclose(got["ap"][t, classes], ap, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["p"][t, classes], p, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["r"][t, classes], r, rtol=0, atol=1e-12)
        assert abs(metrics_ref.maps(got)[t] - float(np.mean(ap))) <= 1e-12


def test_metrics_ref_flags_a_bad_gt_label():
    rec = metrics_ref.Record(3, 1)
    z = (np.zeros((1, 300, 6), np.float32), np.zeros(1, np.int32), np.zeros((1, 1, 300), np.uint8), np.zeros(11), 0.0)
    rec.append(*z, [0.0, 3.0])
    assert rec.status == metrics_ref.BAD_GT_LABEL and rec.gt_hist.tolist() == [1, 0, 0]
    rec = metrics_ref.Record(3, 1)
    rec.append(*z, [1.5, 2.0])
    assert rec.status == metrics_ref.BAD_GT_LABEL and rec.gt_hist.tolist() == [0, 0, 1]


def test_new_kernels_hold_no_spill_and_no_scratch():
    """the figures DESIGN.md records: read from the code object's metadata only"""
    if find_hipcc() is None:
        pytest.skip("hipcc is not on this machine")
    res = kernel_resources(os.path.join(CSRC, "metrics.hip"))
    mine = {k: v for k, v in res.items() if "k_metrics_" in k}
    assert len(mine) == 4, sorted(res)
    for name, k in mine.items():
        print(name[:48], k)
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".max_flat_workgroup_size"] == 256 and k[".vgpr_count"] <= 64, name
    ap = [v for k, v in mine.items() if "k_metrics_ap" in k][0]
    # run bounds 2 int + 4 int + 4 double wave partials + the 256-double staging of the loss
    assert ap[".group_segment_fixed_size"] <= 8 + 16 + 32 + 256 * 8 + 16
