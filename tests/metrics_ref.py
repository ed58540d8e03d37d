"""numpy restatement of the epoch record of csrc/metrics.hip and of what yolat_metrics_finalize computes from it — a
helper of test_metrics_host.py / test_gpu_metrics.py, not a test.

The record: image i of the epoch owns the slots [300 i, 300 i + 300); a slot is (conf fp32, cls int32 with -1 = unfilled,
tp uint32 with bit t = true positive at threshold t).  ``finalize`` is postprocess.ap_per_class + compute_ap
(utils/det_util.py:71-145) per threshold with the one thing numpy leaves open made explicit: equal scores keep slot
order, ``np.argsort(-conf, kind="stable")`` over the filled slots in slot order."""
import numpy as np

SLOTS = 300
BAD_GT_LABEL = 1


def class_of(v, K):
    """the integer class of an fp32 class id, -1 when it is not an integer in [0, K)"""
    v = float(v)
    return int(v) if (0.0 <= v < K and v == np.floor(v)) else -1


class Record(object):
    """The host twin of the device record: ``append`` is yolat_metrics_append(_host) on a batch without flags."""

    def __init__(self, K, T):
        self.K, self.T = K, T
        self.conf, self.cls, self.tp = [], [], []
        self.gt_hist = np.zeros(K, dtype=np.int64)
        self.stats = np.zeros(2 + K * K, dtype=np.int64)
        self.loss, self.status = [], 0

    def append(self, det, det_count, tp, stats, loss, gt_labels):
        det, tp = np.asarray(det, dtype=np.float32), np.asarray(tp)
        B = det.shape[0]
        assert det.shape == (B, SLOTS, 6) and tp.shape == (self.T, B, SLOTS)
        for b in range(B):
            n = min(max(int(det_count[b]), 0), SLOTS)
            conf, cls, mask = np.zeros(SLOTS, np.float32), np.full(SLOTS, -1, np.int32), np.zeros(SLOTS, np.uint32)
            conf[:n] = det[b, :n, 4]
            cls[:n] = [class_of(v, self.K) for v in det[b, :n, 5]]
            for t in range(self.T):
                mask[:n] |= (tp[t, b, :n] != 0).astype(np.uint32) << np.uint32(t)
            self.conf.append(conf)
            self.cls.append(cls)
            self.tp.append(mask)
        for v in np.asarray(gt_labels, dtype=np.float32).reshape(-1):
            c = class_of(v, self.K)
            if c >= 0:
                self.gt_hist[c] += 1
            else:
                self.status |= BAD_GT_LABEL
        self.stats += np.asarray(stats, dtype=np.int64)
        self.loss.append(np.float32(loss))

    def finalize(self):
        return finalize(np.concatenate(self.conf), np.concatenate(self.cls), np.concatenate(self.tp), self.gt_hist, self.T,
                        self.K, self.loss, self.stats, self.status)


def compute_ap(recall, precision):
    """utils/det_util.py:124-145"""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([0.0], precision, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def finalize(conf, cls, tp, gt_hist, T, K, loss=(), stats=None, status=0):
    """-> dict ap / p / r [T, K] float64 (0 for a class without targets or without detections), n_gt / n_p [K] int64,
    loss_mean (the float64 sum of the fp32 losses in index order / their number), stats, status"""
    conf, cls, tp = np.asarray(conf, np.float32), np.asarray(cls, np.int32), np.asarray(tp, np.uint32)
    filled = np.flatnonzero(cls >= 0)                                   # slot order
    order = filled[np.argsort(-(conf[filled] + np.float32(0)), kind="stable")]
    s_cls, s_tp = cls[order], tp[order]
    ap, p, r = (np.zeros((T, K), dtype=np.float64) for _ in range(3))
    n_gt = np.asarray(gt_hist, dtype=np.int64).copy()
    n_p = np.bincount(s_cls, minlength=K).astype(np.int64)[:K]
    for t in range(T):
        flags = ((s_tp >> np.uint32(t)) & np.uint32(1)).astype(np.float64)
        for c in range(K):
            if n_gt[c] == 0 or n_p[c] == 0:
                continue
            f = flags[s_cls == c]
            fpc, tpc = (1 - f).cumsum(), f.cumsum()
            recall, precision = tpc / (n_gt[c] + 1e-16), tpc / (tpc + fpc)
            r[t, c], p[t, c], ap[t, c] = recall[-1], precision[-1], compute_ap(recall, precision)
    total = 0.0
    for v in loss:
        total += float(v)
    return {"ap": ap, "p": p, "r": r, "n_gt": n_gt, "n_p": n_p, "loss_mean": total / max(len(loss), 1),
            "stats": None if stats is None else np.asarray(stats, dtype=np.int64), "status": status}


def maps(res):
    """per threshold the mean AP over the classes with targets (0.0 without any): report["map"]"""
    classes = np.flatnonzero(res["n_gt"] > 0)
    return [float(np.mean(res["ap"][t, classes])) if len(classes) else 0.0 for t in range(res["ap"].shape[0])]
