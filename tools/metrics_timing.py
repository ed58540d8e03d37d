"""Times one ``test()`` epoch end to end on one GPU — 450 batches, the length of the reference's Floorplans test list —
with the metrics computed on the host (``opt.async_eval``: one read per batch, the unpacking, ten numpy ``ap_per_class``
passes) and on the device (``opt.device_metrics``: csrc/metrics.hip, one copy per epoch), and the finalize launch chain
alone next to the ten numpy passes on the same data.

    python tools/metrics_timing.py [--reps 5] [--batches 450] [--parent DIR] [--out profiles/metrics_timing.json]

Workloads: those of tools/evaluate_async_timing.py — one Floorplans-sized item per batch (2000 proposals, 20 targets) and
one cfg-2-sized item per batch (400 proposals, 50 targets), eight distinct HOST batches (``collate``, what a DataLoader hands
to ``test()``) cycled to the epoch's length, ten IoU thresholds.  An epoch is timed from the call of ``test()`` to its
return (the report is on the host then) plus a device synchronise; next to the wall time the record holds the process CPU
seconds of the epoch and the split "loop" (until ``evaluate_stream`` is exhausted) / "final" (what ``test()`` does behind
it: the concatenations and AP passes, or ``EpochMetrics.result()``).  Every repetition is kept, not only a summary.

Three runs, each a process of its own under ``timeout -k 10``, chained — a step that fails or runs out of time ends the
run:  (a) ``--parent DIR``, another checkout of the project with its library built (the commit this change is measured
against), ``opt.async_eval``;  (b) this tree, ``opt.async_eval``, and (c) this tree, ``opt.device_metrics``, alternating
in one process;  then (a) once more, so that (a)'s spread spans the session.  Without --parent only (b) and (c) run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = {
    "floorplans": dict(graph=dict(num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2), targets=20),
    "cfg2": dict(graph=dict(num_proposals=400, nodes_lo=10, nodes_hi=40, edges_per_proposal=100), targets=50),
}
OPTKW = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
STEP_SECONDS = 500
FINALIZE_IMAGES = 450          # 135 000 slots, all filled


def run_child(variants, reps, n_batches, finalize):
    import numpy as np
    import torch

    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv
    from yolat_vectorgraphicsrecognition_amd import evaluation as ev

    marks = []
    orig_stream = ev.evaluate_stream

    def timed_stream(*a, **k):
        yield from orig_stream(*a, **k)
        marks.append(time.perf_counter())

    ev.evaluate_stream = timed_stream
    out = {"device": torch.cuda.get_device_name(0), "workloads": {}}
    for name, spec in WORKLOADS.items():
        rng = np.random.default_rng(7)
        batches = []
        for i in range(8):
            it = yv.synth_graph(seed=1100 + i, with_roots=True, **spec["graph"])
            P = it.bbox.shape[0]
            pick = rng.choice(P, size=spec["targets"], replace=False)
            it.gt_bbox = it.bbox[pick].clone()
            it.gt_labels = torch.from_numpy(rng.integers(0, OPTKW["n_classes"] - 1, size=spec["targets"])).long()
            it.has_obj = torch.ones(P, dtype=torch.long)
            it.width, it.height = torch.tensor([1000.0]), torch.tensor([800.0])
            batches.append(yv.collate([it]))
        model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**OPTKW)), 0).cuda().eval()
        with torch.no_grad():
            d0 = yv.collate_to_device([yv.synth_graph(seed=1100, with_roots=True, **spec["graph"])])
            z = model(*d0)[0]
            gap = z[:, :-1].max(1).values - z[:, -1]
            model.prediction_cls[2][0].bias[model.n_classes - 1] += float(gap.median())

        def epoch(variant, n):
            opt = yv.Opt(**OPTKW)
            opt.async_eval = True
            opt.device_metrics = variant == "device_metrics"
            loader = [batches[i % len(batches)] for i in range(n)]
            del marks[:]
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            value = yv.evaluate(model, loader, yv.DetectionLoss(opt), opt)
            torch.cuda.synchronize()
            t1, c1 = time.perf_counter(), time.process_time()
            return {"wall_s": t1 - t0, "batches_per_sec": n / (t1 - t0), "host_cpu_s": c1 - c0, "loop_s": marks[0] - t0,
                    "final_s": t1 - marks[0]}, value, opt.test_report

        reports = {}
        for v in variants:                                         # warm every path at a tenth of the length
            epoch(v, max(n_batches // 10, 16))
        runs = {v: [] for v in variants}
        for r in range(reps):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                rec, value, rep = epoch(v, n_batches)
                runs[v].append(rec)
                reports[v] = (value, rep)
        w = {"proposals": spec["graph"]["num_proposals"], "targets": spec["targets"], "thresholds": 10, "batches": n_batches,
             "runs": {v: {k: [rec[k] for rec in recs] for k in recs[0]} for v, recs in runs.items()},
             "test_value": {v: reports[v][0] for v in variants}}
        if len(variants) == 2:
            a, b = (reports[v][1] for v in variants)
            w["device_vs_host_report"] = {
                "map_max_abs_diff": float(max(abs(x - y) for x, y in zip(a["map"], b["map"]))),
                "top1_equal": bool(a["top1"] == b["top1"]), "confusion_equal": bool(np.array_equal(a["confusion"], b["confusion"])),
                "loss_abs_diff": float(abs(a["loss"]["loss"] - b["loss"]["loss"]))}
        out["workloads"][name] = w
    if finalize:
        out["finalize_alone"] = finalize_alone(yv, np, torch)
    return out


def finalize_alone(yv, np, torch):
    """the finalize launch chain at 135 000 filled slots between HIP events, and the ten numpy passes on the same data"""
    ops = yv.ops
    K, T, n_img, per = OPTKW["n_classes"], 10, FINALIZE_IMAGES, 50
    rng = np.random.default_rng(11)
    M = n_img * 300
    conf = rng.permutation(M).astype(np.float32) / np.float32(M)      # tie-free: numpy's argsort leaves ties open
    cls = rng.integers(0, K - 1, size=M).astype(np.float32)
    tp = (rng.random((T, M)) < 0.3).astype(np.uint8)
    gt = rng.integers(0, K - 1, size=n_img * 20).astype(np.float32)
    rec = ops.metrics_record(n_img, K, n_img // per, "cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for j in range(n_img // per):
        lo, hi = j * per * 300, (j + 1) * per * 300
        det = np.zeros((per, 300, 6), np.float32)
        det[:, :, 4], det[:, :, 5] = conf[lo:hi].reshape(per, 300), cls[lo:hi].reshape(per, 300)
        tpb = np.ascontiguousarray(tp[:, lo:hi].reshape(T, per, 300))
        ops.metrics_append_host(rec, up(det), up(np.full(per, 300, np.int32)), up(tpb), up(np.zeros(2 + K * K, np.int32)),
                                up(np.zeros(1, np.float32)), up(gt[j::n_img // per]), j * per, j)
    for _ in range(3):
        words = ops.metrics_finalize(rec, n_img, n_img // per, T)
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        words = ops.metrics_finalize(rec, n_img, n_img // per, T)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    host = words.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    got = ops.metrics_unpack(host, T, K, n_img // per)
    host_ms, err = [], 0.0
    for _ in range(5):
        t0 = time.perf_counter()
        aps = [yv.ap_per_class(tp[t].astype(np.float64), conf, cls, gt) for t in range(T)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    for t in range(T):
        err = max(err, float(np.abs(got["ap"][t, aps[t][4]] - aps[t][2]).max()))
    return {"filled_slots": M, "thresholds": T, "classes": K, "finalize_hip_events_ms": dev_ms,
            "copy_of_the_block_ms": copy_ms, "block_bytes": int(host.nbytes), "numpy_ten_ap_per_class_passes_ms": host_ms,
            "ap_max_abs_diff_device_vs_numpy": err}


def spread(v):
    return max(v) - min(v)


def median(v):
    return sorted(v)[len(v) // 2]


def verdict(w):
    """what the three runs show for one workload: every figure a wall time in seconds per epoch"""
    runs = w["runs"]
    b, c = runs["async_eval"]["wall_s"], runs["device_metrics"]["wall_s"]
    out = {"b_median_s": median(b), "c_median_s": median(c), "c_over_b_median": median(c) / median(b)}
    if "parent_async_eval" in runs:
        a = runs["parent_async_eval"]["wall_s"]
        out.update({"a_median_s": median(a), "a_min_s": min(a), "a_max_s": max(a), "a_spread_s": spread(a),
                    "b_median_inside_a_range": bool(min(a) <= median(b) <= max(a)),
                    "c_not_slower_than_a_beyond_a_spread": bool(median(c) <= median(a) + spread(a)),
                    "c_over_a_median": median(c) / median(a)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=450)
    ap.add_argument("--parent", default=None, help="another checkout of the project, built: run (a)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) comma-separated variants to run in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout the child imports")
    ap.add_argument("--finalize", action="store_true", help="(internal) the child also times the finalize chain alone")
    args = ap.parse_args()
    if args.child is not None:
        sys.path.insert(0, os.path.abspath(args.tree))
        sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "tests"))
        rec = run_child(args.child.split(","), args.reps, args.batches, args.finalize)
        with open(args.out, "w") as f:
            json.dump(rec, f)
        return 0
    with tempfile.TemporaryDirectory(prefix="metrics_timing_") as tmp:
        me = "timeout -k 10 %d %s %s --reps %d --batches %d" % (STEP_SECONDS, sys.executable, os.path.abspath(__file__),
                                                                args.reps, args.batches)
        steps, parts = [], []
        if args.parent:
            parts.append(("a1", os.path.join(tmp, "a1.json")))
            steps.append("%s --child async_eval --tree %s --out %s" % (me, os.path.abspath(args.parent), parts[-1][1]))
        parts.append(("bc", os.path.join(tmp, "bc.json")))
        steps.append("%s --child async_eval,device_metrics --finalize --out %s" % (me, parts[-1][1]))
        if args.parent:
            parts.append(("a2", os.path.join(tmp, "a2.json")))
            steps.append("%s --child async_eval --tree %s --out %s" % (me, os.path.abspath(args.parent), parts[-1][1]))
        rc = subprocess.call(" && ".join(steps), shell=True)
        if rc != 0:
            print("a step ended with status %d: nothing written" % rc, file=sys.stderr)
            return rc
        got = {}
        for key, path in parts:
            with open(path) as f:
                got[key] = json.load(f)
    rec = {"unit": "seconds per test() epoch unless named otherwise", "batches_per_epoch": args.batches, "repetitions": args.reps,
           "kw": {"eval_depth": 4, "eval_streams": None, "thresholds": 10}, "device": got["bc"]["device"],
           "order_of_the_runs": [k for k, _ in parts], "workloads": {}, "finalize_alone": got["bc"]["finalize_alone"]}
    for name, w in got["bc"]["workloads"].items():
        if args.parent:
            a1, a2 = (got[k]["workloads"][name]["runs"]["async_eval"] for k in ("a1", "a2"))
            w["runs"]["parent_async_eval"] = {k: a1[k] + a2[k] for k in a1}
            w["test_value"]["parent_async_eval"] = got["a1"]["workloads"][name]["test_value"]["async_eval"]
        w["what_the_runs_show"] = verdict(w)
        rec["workloads"][name] = w
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
