"""Times the device augmentation (csrc/augment.hip, yolat_augment_batch) at the batch shapes of cfg 3 (4 graphs x 2000
proposals of 4 - 40 nodes) and cfg 4 (32 graphs x 300 proposals of 4 - 24 nodes) — and at 16 times the cfg-3 batch, where
the launch is long enough to show its streaming rate — in ONE process:

  launch_us        HIP-event time of the one launch (warm; --reps launches between two events, median of --runs windows;
                   the entry point is called directly, so that the host enqueues faster than the device executes)
  call_us          host wall clock of augment.augment_batch_ (parameter upload + launch), device synchronised at both ends
  torch_us         the same result composed from torch operations: an index by graph-of-node, element-wise float64
                   operations, four scatter_reduce calls (events, same windows)
  copy_GBps        read + written bytes per second of a plain device copy of 256 MiB in this process
  bytes, fraction  the launch's traffic (8 N + 4 P read, 16 N + 16 P written) and bytes / launch time over the copy rate

The timed launches use the drawn rotation and flips with scale 1 and no translation, so that hundreds of in-place
applications keep the coordinates bounded; the arithmetic per node is the same.  Before timing, one application with the
drawn parameters is checked bit for bit against the torch composition.

  python tools/augment_timing.py --out profiles/augment_timing.json
Prints one JSON line; --out also writes it to a file.  Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def items_of(yv, shape):
    if shape == "cfg3_x16":  # 64 graphs of the cfg-3 item size: where the launch is long enough to be a stream
        return [yv.synth_graph(seed=5000 + i, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, augmented=True)
                for i in range(64)]
    if shape == "cfg3":      # data.config("3")
        return [yv.synth_graph(seed=3000 + i, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, augmented=True)
                for i in range(4)]
    return [yv.synth_graph(seed=4000 + i, num_proposals=300, nodes_lo=4, nodes_hi=24, edge_factor=1.2, n_classes=22,
                           augmented=True) for i in range(32)]


def torch_composition(pos, x, bbox, node_graph, node_prop, blk):
    """random_transfer + update_bbox from torch operations, in place like the launch; blk [B, 8] float64 on the device"""
    q = blk[node_graph]                                       # indexing: the graph's row for every node
    c, s, scale, tx, ty = q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4]
    p = pos.double() - 0.5
    px = torch.where(q[:, 5] != 0, -p[:, 0], p[:, 0])
    py = torch.where(q[:, 6] != 0, -p[:, 1], p[:, 1])
    rx = px * c + py * (-s)
    ry = px * s + py * c
    rx = rx + 0.5 + tx
    ry = ry + 0.5 + ty
    ox = (rx * scale + ry * 0.0).float()
    oy = (rx * 0.0 + ry * scale).float()
    pos[:, 0], pos[:, 1] = ox, oy
    x[:, 3], x[:, 4] = ox, oy
    P = bbox.shape[0]
    inf = float("inf")
    lo_x = torch.full((P,), inf, device=pos.device).scatter_reduce(0, node_prop, ox, "amin")
    lo_y = torch.full((P,), inf, device=pos.device).scatter_reduce(0, node_prop, oy, "amin")
    hi_x = torch.full((P,), -inf, device=pos.device).scatter_reduce(0, node_prop, ox, "amax")
    hi_y = torch.full((P,), -inf, device=pos.device).scatter_reduce(0, node_prop, oy, "amax")
    bbox.copy_(torch.stack([lo_x, lo_y, hi_x, hi_y], 1))


def event_windows(fn, reps, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return out


def copy_rate(runs):
    n = 256 << 20
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.zero_()
    us = statistics.median(event_windows(lambda: dst.copy_(src), 20, runs, 5))
    return 2.0 * n / (us * 1e-6) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_timing needs the GPU")
    import yolat_vectorgraphicsrecognition_amd as yv
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": a.runs}
    res["copy_GBps"] = copy_rate(a.runs)
    for shape in ("cfg3", "cfg4", "cfg3_x16"):
        items = items_of(yv, shape)
        B = len(items)
        np.random.seed(5)
        random.seed(5)
        params = yv.draw_params(B)
        batch, slices = yv.collate_to_device(items, csr=True)
        g = batch._yolat_graph
        pos, x, bbox = batch.pos, batch.x, batch.bbox
        N, P = pos.shape[0], bbox.shape[0]
        node_prop = g.node_seg.long()
        prop = slices["labels"].cuda()
        node_graph = torch.bucketize(node_prop, prop[1:], right=True)
        blk = torch.from_numpy(params.block()).cuda()
        # one application with the drawn parameters: launch == composition, bit for bit
        p1, x1, b1 = pos.clone(), x.clone(), bbox.clone()
        torch_composition(p1, x1, b1, node_graph, node_prop, blk)
        yv.augment_batch_(batch, slices, params)
        torch.cuda.synchronize()
        same = bool(torch.equal(p1, pos) and torch.equal(x1, x) and torch.equal(b1, bbox))
        # timed: rotation and flips only (bounded under repetition)
        calm = yv.AugParams(np.ones(B), params.angle, np.zeros((B, 2)), params.flips)
        cblk = torch.from_numpy(calm.block()).cuda()
        args = (pos.data_ptr(), x.data_ptr(), x.stride(0), 3, 4, g.seg_ptr.data_ptr(), prop.data_ptr(), bbox.data_ptr(),
                cblk.data_ptr(), N, P, B, ops._stream())
        ops.augment_batch(pos, x, g.seg_ptr, prop, bbox, cblk)          # the checked wrapper once: same operands
        launch = event_windows(lambda: lib.yolat_augment_batch(*args), a.reps, a.runs, 20)
        comp = event_windows(lambda: torch_composition(pos, x, bbox, node_graph, node_prop, cblk), max(a.reps // 4, 10),
                             a.runs, 5)
        calls = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                yv.augment_batch_(batch, slices, calm)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e6 / 20)
        nbytes = 8 * N + 4 * P + 16 * N + 16 * P
        lus = statistics.median(launch)
        res[shape] = {"graphs": B, "N": int(N), "P": int(P), "bytes": int(nbytes), "launch_equals_torch_composition": same,
                      "launch_us": lus, "launch_us_min_max": [min(launch), max(launch)],
                      "torch_us": statistics.median(comp), "torch_us_min_max": [min(comp), max(comp)],
                      "call_us": statistics.median(calls),
                      "launch_GBps": nbytes / (lus * 1e-6) / 1e9,
                      "fraction_of_copy_rate": nbytes / (lus * 1e-6) / 1e9 / res["copy_GBps"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
