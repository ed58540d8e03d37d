"""Generates tests/golden/detect.npz.  DEV-TIME ONLY (needs the reference checkout, like make_golden_post.py, whose
helpers it uses); never imported by tests.  Run from the repo root:  python tests/golden/make_golden_detect.py

A 3-image batch with unequal row counts through the reference's OWN ``non_max_suppression`` (compiled from its source
text, oracle_np.nms standing in for torchvision's) — the shorter images padded with zero-objectness rows, which the
reference drops before anything else — and the reference's ``get_batch_statistics`` (utils/det_util.py, imported as
is) on those detections at the ten thresholds of np.linspace(0.5, 0.95, 10).  Data only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_post as mgp          # noqa: E402


def main():
    out = {}
    ref_nms = mgp.reference_nms_function()
    spec = importlib.util.spec_from_file_location("ref_det_util", os.path.join(mgp.REF, "utils", "det_util.py"))
    du = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(du)
    rng = np.random.default_rng(11)
    nc, conf, iou = 12, 0.05, 0.5
    counts = [250, 90, 400]
    rows = [mgp.synth_prediction(rng, n, nc)[0] for n in counts]
    padded = np.zeros((3, max(counts), 5 + nc), dtype=np.float32)
    for i, r in enumerate(rows):
        padded[i, :len(r)] = r
    dets = ref_nms(torch.from_numpy(padded.copy()), conf_thres=conf, iou_thres=iou)
    out["pred"] = np.concatenate(rows, 0)
    out["image_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out["args"] = np.array([conf, iou], dtype=np.float64)
    targets = []
    for i, d in enumerate(dets):
        out["out_%d" % i] = d.numpy()
        k = 20
        pick = rng.choice(d.shape[0], size=k, replace=False)
        tb = d[pick, :4].numpy() + rng.normal(0, 3.0, size=(k, 4)).astype(np.float32)
        tl = d[pick, 5].numpy()
        tb = np.concatenate([tb, tb[:4] + 1.5]).astype(np.float32)          # repeated labels on overlapping targets
        tl = np.concatenate([tl, tl[:4]]).astype(np.float32)
        targets.append(np.concatenate([np.full((len(tb), 1), i, np.float32), tl[:, None], tb], 1))
        print("image %d: %d rows -> %d detections, %d targets" % (i, counts[i], d.shape[0], len(tb)))
    targets = np.concatenate(targets, 0).astype(np.float32)
    out["targets"] = targets
    out["gt_ptr"] = np.searchsorted(targets[:, 0], np.arange(4)).astype(np.int64)
    ths = np.linspace(0.5, 0.95, 10)
    out["thresholds"] = ths
    for t, th in enumerate(ths):
        m = du.get_batch_statistics(list(dets), torch.from_numpy(targets), iou_threshold=th)
        for i in range(3):
            out["tp_%d_%d" % (t, i)] = m[i][0]
        print("threshold %.2f: %s true positives" % (th, [int(m[i][0].sum()) for i in range(3)]))
    np.savez_compressed(os.path.join(HERE, "detect.npz"), **out)
    print("detect: %d arrays" % len(out))


if __name__ == "__main__":
    main()
