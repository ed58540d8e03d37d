"""Times the detection loop of one process on one GPU: the synchronous ``detect_batch`` loop (predict -> scores -> batched NMS,
two host reads per batch) next to ``detect_stream`` (yolat_detect, no host read until the boxes are wanted) at depth 1, 2,
4 and 8.

    python tools/detect_async_timing.py [--rounds 7] [--batches 400] [--out profiles/detect_async_timing.json]

Workloads: one Floorplans-sized item per batch (bench.py's predict leg: 2000 proposals, 4..40 nodes each) and one
cfg-2-sized item per batch (400 proposals, ~10 000 nodes, 40 000 edges), both with proposal trees and a classifier bias
that selects about half of the children.  Eight distinct device batches per workload are cycled, so both loops find the
flattened tree cached on the batch.  Every variant is timed in every round, the rounds alternate the variants, and a window
is `--batches` batches ending in a device synchronise; the record holds min / median / max over the rounds (batches per
second), the detections of the two loops compared bit for bit, the host time of one submission with the device drained
(the enqueue alone) next to the time until its result is there, and the launches per batch of both loops as the torch
profiler's device-side kernel / copy records count them (a run of its own behind the timed rounds)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import golden_util as gu
import yolat_vectorgraphicsrecognition_amd as yv

WORKLOADS = {
    "floorplans": dict(num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2),
    "cfg2": dict(num_proposals=400, nodes_lo=10, nodes_hi=40, edges_per_proposal=100),
}
OPTKW = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
KW = dict(conf_thres=0.25, iou_thres=0.45)


def stats(v):
    v = sorted(v)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def build(name):
    batches = [yv.collate_to_device([yv.synth_graph(seed=1100 + i, with_roots=True, **WORKLOADS[name])]) for i in range(8)]
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**OPTKW)), 0).cuda().eval()
    with torch.no_grad():
        z = model(*batches[0])[0]
        gap = z[:, :-1].max(1).values - z[:, -1]
        model.prediction_cls[2][0].bias[model.n_classes - 1] += float(gap.median())
    return model, batches


def sync_loop(model, batches, n):
    out = None
    for i in range(n):
        out = yv.detect_batch(model, *batches[i % len(batches)], fixup=False, **KW)
    torch.cuda.synchronize()
    return out


def stream_loop(model, batches, n, depth):
    out = None
    for out in yv.detect_stream(model, (batches[i % len(batches)] for i in range(n)), depth=depth, **KW):
        pass
    torch.cuda.synchronize()
    return out


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
                if "memcpy" in ev.name.lower() or "copy" in ev.name.lower() and "kernel" not in ev.name.lower():
                    copies += 1
                else:
                    kernels += 1
        return {"kernels": kernels, "copies": copies}
    except Exception as e:      # noqa: BLE001  (a box without the tracer: the timing still stands)
        return {"error": "%s: %s" % (type(e).__name__, e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "batches_per_window": args.batches,
           "unit": "batches per second (one item per batch)", "kw": KW, "workloads": {}}
    for name in WORKLOADS:
        model, batches = build(name)
        d0, s0 = batches[0]
        variants = [("sync_detect_batch", lambda n: sync_loop(model, batches, n))]
        for depth in (1, 2, 4, 8):
            variants.append(("stream_depth%d" % depth, lambda n, depth=depth: stream_loop(model, batches, n, depth)))
        rates = {v[0]: [] for v in variants}
        same = True
        for key, fn in variants:                           # warm every variant, and compare what they return
            got = fn(len(batches) * 2)
            want = sync_loop(model, batches, len(batches) * 2)
            same = same and len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
        for r in range(args.rounds):
            order = variants if r % 2 == 0 else variants[::-1]
            for key, fn in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(args.batches)
                rates[key].append(args.batches / (time.perf_counter() - t0))
        submit_ms, done_ms = [], []
        for i in range(50):                                # one submission at a time, device drained in front of each
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = yv.detect_batch_async(model, *batches[i % len(batches)], fixup=False, **KW)
            t1 = time.perf_counter()
            h.result()
            submit_ms.append((t1 - t0) * 1e3)
            done_ms.append((time.perf_counter() - t0) * 1e3)
        w = {"proposals": int(d0.bbox.shape[0]), "nodes": int(d0.x.shape[0]), "edges": int(d0.edge.shape[0]),
             "roots": len(d0.roots), "tree_nodes": len(d0.roots) + sum(len(r.children) for r in d0.roots),
             "bit_identical_detections": bool(same), "batches_per_sec": {k: stats(v) for k, v in rates.items()}}
        sync = w["batches_per_sec"]["sync_detect_batch"]
        w["sync_spread_frac"] = (sync["max"] - sync["min"]) / sync["median"]
        w["speedup_median_over_sync"] = {k: v["median"] / sync["median"] for k, v in w["batches_per_sec"].items()}
        w["one_submission_ms"] = {"host_enqueue": stats(submit_ms), "until_result": stats(done_ms)}
        w["launches_per_batch"] = {
            "sync_detect_batch": launches(lambda: yv.detect_batch(model, d0, s0, fixup=False, **KW)),
            "detect_submit_result": launches(lambda: yv.detect_batch_async(model, d0, s0, fixup=False, **KW).result()),
        }
        rec["workloads"][name] = w
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
