"""Times a classifier = 'sigmoid' model next to the softmax model on the two paths the classifier switch used to push off
the fast lane: the cfg-3 training step (ms per step with the GPU drained after every step, host ms per step = enqueue
only, and how many steps went through yolat_train_step) and predict() on one Floorplans-sized item (ms per call, timed
like bench.py's predict leg).  One JSON line.

    python tools/sigmoid_timing.py [--classifiers softmax,sigmoid] [--steps 40]

YOLAT_TIMING_ROOT: a checkout to import the package (and tests/golden_util.py) from instead of this one — the same
script against another commit's build on the same box in the same session."""
import argparse
import json
import os
import sys
import time

ROOT = os.environ.get("YOLAT_TIMING_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import golden_util as gu
import yolat_vectorgraphicsrecognition_amd as yv


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def train_times(classifier, steps):
    data, slices, optkw, _ = yv.config("3")
    opt = yv.Opt(**dict(optkw, classifier=classifier))
    model = gu.fill_state_(yv.SparseCADGCN(opt), 0).cuda()
    for k in ("x", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
        setattr(data, k, getattr(data, k).cuda())
    tr = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5)
    for _ in range(5):
        tr.step(data, slices)
    torch.cuda.synchronize()
    wall, host = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        tr.step(data, slices)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3)
        wall.append((t2 - t0) * 1e3)
    return {"ms_per_step": _median(wall), "host_ms_per_step": _median(host), "plan_steps": tr.plan_steps,
            "steps": tr._steps}


def predict_times(classifier, budget_s=2.0):
    optkw = dict(n_classes=17, n_blocks=2, n_blocks_out=2, classifier=classifier)
    data, slices = yv.synth_batch(1, 11, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, with_roots=True)
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 0).cuda().eval()
    calls = []
    orig = model._predict_two_pass
    model._predict_two_pass = lambda d, s: calls.append(1) or orig(d, s)

    def one():
        with torch.no_grad():
            return model.predict(data, slices)

    for _ in range(3):
        out = one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one()
    torch.cuda.synchronize()
    n = int(max(8, min(200, budget_s / max(time.perf_counter() - t0, 1e-5))))
    chunk = max(1, n // 4)
    means = []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(chunk):
            one()
        torch.cuda.synchronize()
        means.append((time.perf_counter() - t0) / chunk)
    means.sort()
    return {"ms_per_call": 0.5 * (means[1] + means[2]) * 1e3, "rows": int(out[0].shape[0]),
            "two_pass_calls": len(calls), "calls": 4 + 4 * chunk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classifiers", default="softmax,sigmoid")
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    rec = {"package": os.path.dirname(os.path.abspath(yv.__file__)), "device": torch.cuda.get_device_name(0)}
    for c in args.classifiers.split(","):
        rec[c] = {"train_cfg3": train_times(c, args.steps), "predict_floorplans": predict_times(c)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
