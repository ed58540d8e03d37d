"""Times the evaluation loop of one process on one GPU: the synchronous ``evaluate_batch(device_post=True)`` loop (predict,
loss, top-1, scores, NMS, true-positive walk: five synchronising reads and two uploads per batch) next to
``evaluate_stream`` (yolat_evaluate, one read per batch when its dict is wanted) at depth 4 on one stream and on three.

    python tools/evaluate_async_timing.py [--rounds 7] [--batches 200] [--out profiles/evaluate_async_timing.json]

Workloads: one Floorplans-sized item per batch (2000 proposals, 4..40 nodes each, 20 targets) and one cfg-2-sized item
per batch (400 proposals, ~10 000 nodes, 40 000 edges, 50 targets), both with proposal trees, a classifier bias that
selects about half of the children, and the ten IoU thresholds 0.5 .. 0.95.  Eight distinct device batches per workload
are cycled, so every loop finds its uploads cached on the batch (the synchronous loop gets its batch's labels and proposal
offsets put back in front of every call: evaluate_batch overwrites them).  Every loop is timed in every round, the rounds
alternate the order, and a window is `--batches` batches ending in a device synchronise; the record holds min / median /
max over the rounds (batches per second), the dicts of the loops compared with the synchronous loop's, the host time of one
submission with the device drained next to the time until its result is there, and the launches and copies per batch of
both paths as the torch profiler's device-side records count them (a run of its own behind the timed rounds).

Each workload is a GPU step of its own: without --workload this process starts one child per workload under
``timeout -k 10``, chained with ``&&`` — a step that fails or runs out of time ends the run — and merges their records."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = {
    "floorplans": dict(graph=dict(num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2), targets=20),
    "cfg2": dict(graph=dict(num_proposals=400, nodes_lo=10, nodes_hi=40, edges_per_proposal=100), targets=50),
}
OPTKW = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
STEP_SECONDS = 900


def stats(v):
    v = sorted(v)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def run_workload(name, rounds, n_batches):
    import numpy as np
    import torch

    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv

    spec = WORKLOADS[name]
    rng = np.random.default_rng(7)
    batches = []
    for i in range(8):
        it = yv.synth_graph(seed=1100 + i, with_roots=True, **spec["graph"])
        P = it.bbox.shape[0]
        pick = rng.choice(P, size=spec["targets"], replace=False)
        it.gt_bbox = it.bbox[pick].clone()
        it.gt_labels = torch.from_numpy(rng.integers(0, OPTKW["n_classes"] - 1, size=spec["targets"])).long()
        it.width, it.height = torch.tensor([1000.0]), torch.tensor([800.0])
        batches.append(yv.collate_to_device([it]))
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**OPTKW)), 0).cuda().eval()
    with torch.no_grad():
        z = model(*batches[0])[0]
        gap = z[:, :-1].max(1).values - z[:, -1]
        model.prediction_cls[2][0].bias[model.n_classes - 1] += float(gap.median())
    crit = yv.DetectionLoss(yv.Opt(**OPTKW))
    keep = [(d.labels, s["bbox"]) for d, s in batches]
    three = [torch.cuda.Stream() for _ in range(3)]

    def sync_one(i):
        d, s = batches[i % len(batches)]
        d.labels, s["bbox"] = keep[i % len(batches)]
        with torch.no_grad():
            return yv.evaluate_batch(model, crit, d, s, fixup=False, device_post=True)

    def sync_loop(n):
        out = [sync_one(i) for i in range(n)]
        torch.cuda.synchronize()
        return out

    def stream_loop(n, streams):
        for i in range(len(batches)):
            batches[i][0].labels, batches[i][1]["bbox"] = keep[i]
        out = list(yv.evaluate_stream(model, (batches[i % len(batches)] for i in range(n)), depth=4, streams=streams))
        torch.cuda.synchronize()
        return out

    def same(a, b):
        if len(a) != len(b):
            return False
        for g, w in zip(a, b):
            ok = g["loss"] == w["loss"] and g["n_true"] == w["n_true"] and g["n_total"] == w["n_total"] and \
                g["labels"] == w["labels"] and np.array_equal(g["y_pred"], w["y_pred"]) and np.array_equal(g["y_true"], w["y_true"])
            for mg, mw in zip(g["sample_metrics"], w["sample_metrics"]):
                for (tg, sg, lg), (tw, sw, lw) in zip(mg, mw):
                    ok = ok and np.array_equal(tg, tw) and np.asarray(sg).tobytes() == np.asarray(sw).tobytes() and \
                        np.asarray(lg).tobytes() == np.asarray(lw).tobytes()
            if not ok:
                return False
        return True

    def launches(fn):
        """device-side kernel and copy records of one call of fn, as the torch profiler sees them; None when it cannot"""
        try:
            from torch.profiler import profile, ProfilerActivity
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            kernels = copies = 0
            for ev in prof.events():
                if str(getattr(ev, "device_type", "")).endswith("CUDA"):
                    low = ev.name.lower()
                    if "memcpy" in low or "memset" in low or ("copy" in low and "kernel" not in low):
                        copies += 1
                    else:
                        kernels += 1
            return {"kernels": kernels, "copies_and_memsets": copies}
        except Exception as e:      # noqa: BLE001  (a box without the tracer: the timing still stands)
            return {"error": "%s: %s" % (type(e).__name__, e)}

    variants = [("sync_evaluate_batch", sync_loop), ("stream_depth4_one_stream", lambda n: stream_loop(n, None)),
                ("stream_depth4_three_streams", lambda n: stream_loop(n, three))]
    want = sync_loop(len(batches) * 2)
    identical = {key: bool(same(fn(len(batches) * 2), want)) for key, fn in variants}      # (this also warms every loop)
    rates = {key: [] for key, _ in variants}
    for r in range(rounds):
        for key, fn in (variants if r % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n_batches)
            rates[key].append(n_batches / (time.perf_counter() - t0))
    submit_ms, done_ms = [], []
    for i in range(len(batches)):
        batches[i][0].labels, batches[i][1]["bbox"] = keep[i]
    for i in range(50):                                    # one submission at a time, device drained in front of each
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = yv.evaluate_batch_async(model, *batches[i % len(batches)], fixup=False)
        t1 = time.perf_counter()
        h.result()
        submit_ms.append((t1 - t0) * 1e3)
        done_ms.append((time.perf_counter() - t0) * 1e3)
    d0, s0 = batches[0]
    w = {"proposals": int(d0.bbox.shape[0]), "nodes": int(d0.x.shape[0]), "edges": int(d0.edge.shape[0]),
         "roots": len(d0.roots), "tree_nodes": len(d0.roots) + sum(len(r.children) for r in d0.roots),
         "targets": spec["targets"], "thresholds": 10, "equal_to_the_synchronous_dicts": identical,
         "batches_per_sec": {k: stats(v) for k, v in rates.items()}}
    sync = w["batches_per_sec"]["sync_evaluate_batch"]
    w["sync_spread_frac"] = (sync["max"] - sync["min"]) / sync["median"]
    w["speedup_median_over_sync"] = {k: v["median"] / sync["median"] for k, v in w["batches_per_sec"].items()}
    w["one_stream_median_clears_sync_max"] = bool(w["batches_per_sec"]["stream_depth4_one_stream"]["median"] > sync["max"])
    w["one_submission_ms"] = {"host_enqueue": stats(submit_ms), "until_result": stats(done_ms)}
    w["launches_per_batch"] = {"sync_evaluate_batch": launches(lambda: sync_one(0))}
    d0.labels, s0["bbox"] = keep[0]
    w["launches_per_batch"]["evaluate_submit_result"] = \
        launches(lambda: yv.evaluate_batch_async(model, d0, s0, fixup=False).result())
    return {"device": torch.cuda.get_device_name(0), "workload": w}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", default=None, help="(internal) run this one workload and write its record to --out")
    args = ap.parse_args()
    if args.workload is not None:
        rec = run_workload(args.workload, args.rounds, args.batches)
        with open(args.out, "w") as f:
            json.dump(rec, f)
        return 0
    with tempfile.TemporaryDirectory(prefix="eval_timing_") as tmp:
        parts = {name: os.path.join(tmp, name + ".json") for name in WORKLOADS}
        steps = ["timeout -k 10 %d %s %s --rounds %d --batches %d --workload %s --out %s"
                 % (STEP_SECONDS, sys.executable, os.path.abspath(__file__), args.rounds, args.batches, name, path)
                 for name, path in parts.items()]
        rc = subprocess.call(" && ".join(steps), shell=True)
        if rc != 0:
            print("a step ended with status %d: nothing written" % rc, file=sys.stderr)
            return rc
        rec = {"rounds": args.rounds, "batches_per_window": args.batches, "unit": "batches per second (one item per batch)",
               "kw": {"conf_thres": 0.0, "iou_thres": 0.5, "depth": 4}, "workloads": {}}
        for name, path in parts.items():
            with open(path) as f:
                part = json.load(f)
            rec["device"] = part["device"]
            rec["workloads"][name] = part["workload"]
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
