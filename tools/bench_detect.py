"""Times the detection post-processing of one evaluation batch: everything evaluation.evaluate_batch does after
``model.predict`` and the loss — per image from Python (the default path) against the three device calls of
``device_post=True`` (csrc/detect.hip) plus their host unpacking.  Wall clock, device synchronised at both ends, warm,
median of --reps repetitions, --runs runs.

Batch: 8 Floorplans-sized items (the item of bench.py's predict leg), n_classes = 17, 50 ground-truth boxes per image
picked from the image's own proposals, the ten IoU thresholds of the evaluation loop.

  python tools/bench_detect.py --out profiles/detect_post_timing.json          both paths + the 30 000-candidate case
  python tools/bench_detect.py --path old --out old.json                       the default path alone (runs on a checkout
                                                                               that has no device path, e.g. the parent)
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def build_batch(yv, n_images, n_gt, seed=11):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n_images):
        it = yv.synth_graph(seed=seed * 1000 + i, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, with_roots=True)
        P = it.bbox.shape[0]
        pick = rng.choice(P, size=min(n_gt, P), replace=False)
        it.gt_bbox = it.bbox[pick].clone()
        it.gt_labels = torch.from_numpy(rng.integers(0, 16, size=len(pick))).long()
        it.has_obj = torch.ones(P, dtype=torch.long)
        it.width = torch.tensor([1000.0])
        it.height = torch.tensor([800.0])
        items.append(it)
    return yv.collate(items)


def old_post(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths):
    """evaluation.evaluate_batch, default path: the per-image loop after predict and the loss."""
    metrics = [[] for _ in ths]
    for i in range(len(image_ptr) - 1):
        pc = pred_cls[image_ptr[i]:image_ptr[i + 1]]
        pb = pred_coord[image_ptr[i]:image_ptr[i + 1]]
        w, h = float(data.width[i]), float(data.height[i])
        scale = torch.tensor([w, h, w, h], dtype=pb.dtype, device=pb.device)
        gt = data.gt_bbox[int(label_ptr[i]):int(label_ptr[i + 1])].float() * scale.cpu()
        gl = data.gt_labels[int(label_ptr[i]):int(label_ptr[i + 1])]
        targets = torch.cat((torch.zeros(gl.shape[0], 1), gl.float().unsqueeze(1), gt), 1)
        pc = torch.softmax(pc, dim=1)
        conf = torch.cat((1 - pc[:, -1:], pc[:, :-1]), 1)
        pred = torch.cat((pb * scale, conf), 1).unsqueeze(0)
        outputs = [o.cpu() for o in yv.non_max_suppression(pred, conf_thres=0.0, iou_thres=0.5)]
        for t, th in enumerate(ths):
            metrics[t] += yv.get_batch_statistics(outputs, targets, iou_threshold=th)
    return metrics


def host_inputs(data, image_ptr, label_ptr):
    scales, gts = [], []
    for i in range(len(image_ptr) - 1):
        w, h = float(data.width[i]), float(data.height[i])
        scale = torch.tensor([w, h, w, h], dtype=torch.float32)
        gt = data.gt_bbox[int(label_ptr[i]):int(label_ptr[i + 1])].float() * scale
        gl = data.gt_labels[int(label_ptr[i]):int(label_ptr[i + 1])]
        scales.append(scale)
        gts.append(torch.cat((gl.float().unsqueeze(1), gt), 1))
    return torch.stack(scales).numpy(), torch.cat(gts, 0).numpy()


def new_post(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths):
    """evaluation.evaluate_batch(device_post=True): host inputs, one upload, three calls, one read-back, unpacking."""
    from yolat_vectorgraphicsrecognition_amd.postprocess import detect_post_device
    scales, gts = host_inputs(data, image_ptr, label_ptr)
    return detect_post_device(pred_cls, pred_coord, image_ptr, scales, gts, label_ptr, ths, softmax=True, conf_thres=0.0,
                              iou_thres=0.5)


def wall_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def stage_times(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths, reps):
    """Device time of each of the three calls of the new path (hip events on the stream), inputs resident."""
    dev = pred_cls.device
    scales, gts = host_inputs(data, image_ptr, label_ptr)
    i32 = lambda v: torch.as_tensor(np.asarray([int(x) for x in v], dtype=np.int32)).to(dev)
    iptr, gptr = i32(image_ptr), i32(label_ptr)
    sc, gt = torch.from_numpy(scales).to(dev), torch.from_numpy(gts).to(dev)
    gbox, glab = gt[:, 1:5].contiguous(), gt[:, 0].contiguous()
    th = torch.from_numpy(np.asarray(ths, dtype=np.float32)).to(dev)
    pred = yv.ops.detect_scores(pred_cls, pred_coord, iptr, sc)
    det, cnt = yv.ops.nms_batched(pred, iptr, 0.0, 0.5)
    return {"scores_ms": event_ms(lambda: yv.ops.detect_scores(pred_cls, pred_coord, iptr, sc), reps),
            "nms_batched_ms": event_ms(lambda: yv.ops.nms_batched(pred, iptr, 0.0, 0.5), reps),
            "match_ms": event_ms(lambda: yv.ops.detect_match(det, cnt, gbox, glab, gptr, th), reps),
            "detections": [int(v) for v in cnt.tolist()]}


def single_image_cap(yv, reps, n_centers=3750, spread=8.0, wh=(10.0, 50.0)):
    """One image of 30 000 candidates (the reference's max_nms): ops.nms against nms_batched on the same boxes.
    The default: sparse clusters, thousands of boxes survive and the walk ends at the 300th keep inside the first chunk;
    40 tight clusters of similar boxes: fewer than 300 survive, so all 30 chunks are walked."""
    rng = np.random.default_rng(3)
    n = 30000
    centers = rng.random((n_centers, 2)) * 3000.0
    c = centers[rng.integers(0, len(centers), size=n)] + rng.normal(0, spread, size=(n, 2))
    wh = wh[0] + rng.random((n, 2)) * wh[1]
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = ((rng.permutation(n) + 1) / 32768.0).astype(np.float32)
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    pred = torch.cat((b, torch.ones(n, 1, device="cuda"), s[:, None]), 1).contiguous()
    ptr = torch.tensor([0, n], dtype=torch.int32).cuda()
    keep = yv.ops.nms(b, s, 0.5)
    det, cnt = yv.ops.nms_batched(pred, ptr, 0.0, 0.5, True)
    same = bool(torch.equal(det[0, :int(cnt[0]), :4], b[keep[:300]]))
    return {"n": n, "kept_by_ops_nms": int(keep.shape[0]), "first_300_equal": same,
            "ops_nms_wall_ms": wall_ms(lambda: yv.ops.nms(b, s, 0.5), reps),
            "nms_batched_device_ms": event_ms(lambda: yv.ops.nms_batched(pred, ptr, 0.0, 0.5, True), reps),
            "nms_batched_wall_ms": wall_ms(lambda: yv.ops.nms_batched(pred, ptr, 0.0, 0.5, True)[1].cpu(), reps),
            "ops_nms_work_bytes": int(yv._lib.lib.yolat_nms_work_bytes(n)),
            "nms_batched_work_bytes": int(yv.ops.nms_batched_work_bytes(n, 1, 1)) if hasattr(yv.ops, "nms_batched") else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["both", "old", "new"], default="both")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--gt", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import yolat_vectorgraphicsrecognition_amd as yv
    import golden_util as gu
    assert torch.cuda.is_available(), "bench_detect needs the GPU"
    opt = yv.Opt(n_classes=17, n_blocks=2, n_blocks_out=2)
    model = gu.fill_state_(yv.SparseCADGCN(opt), 5).cuda().eval()
    data, slices = build_batch(yv, args.images, args.gt)
    yv.fixup_offsets(data, slices)
    data.edge_control = None
    with torch.no_grad():
        out = model.predict(data, slices)
    pred_cls, pred_coord = out[0].detach().float(), out[1].detach().float().clone()
    image_ptr, label_ptr = [int(v) for v in out[4]], slices["gt_labels"]
    ths = np.linspace(0.5, 0.95, 10)
    rec = {"workload": "post-processing of one evaluation batch (after predict and the loss)", "images": args.images,
           "rows": int(pred_cls.shape[0]), "classes": int(pred_cls.shape[1]), "gt_per_image": args.gt, "thresholds": len(ths),
           "reps": args.reps, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    paths = {"old": old_post, "new": new_post}
    for name in (("old", "new") if args.path == "both" else (args.path,)):
        fn = paths[name]
        runs = [wall_ms(lambda: fn(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths), args.reps)
                for _ in range(args.runs)]
        rec[name + "_ms_runs"] = runs
        rec[name + "_ms"] = statistics.median(runs)
    if args.path == "both":
        rec["speedup"] = rec["old_ms"] / rec["new_ms"]
        rec["slowest_new_below_fastest_old"] = max(rec["new_ms_runs"]) < min(rec["old_ms_runs"])
        a = old_post(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths)
        b = new_post(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths)
        rec["true_positives_old"] = [int(sum(m[0].sum() for m in a[t])) for t in range(len(ths))]
        rec["true_positives_new"] = [int(sum(m[0].sum() for m in b[t])) for t in range(len(ths))]
    if args.path != "old":
        rec["new_stages"] = stage_times(yv, pred_cls, pred_coord, data, image_ptr, label_ptr, ths, args.reps)
        rec["single_image_30000"] = single_image_cap(yv, args.reps)
        rec["single_image_30000_dense"] = single_image_cap(yv, args.reps, n_centers=40, spread=2.0, wh=(40.0, 10.0))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
