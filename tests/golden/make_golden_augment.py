"""Generates tests/golden/augment.npz from the REFERENCE'S OWN training augmentation: `SESYDFloorPlan.random_transfer`
(Datasets/graph_dict3.py:283-298) with `__transform__` (:236-258) and `__transform_bbox__` (:260-281), followed by the
`update_bbox` that `__getitem__` defines and calls after it (:934-959).  Development-time only; the fixture travels.

    python tests/golden/make_golden_augment.py <reference checkout>            (or YOLAT_REFERENCE=<reference checkout>)
    python tests/golden/make_golden_augment.py <reference checkout> --time     also writes reference_timings_augment.json

The four functions are compiled from the reference's source text where it lies (graph_dict3.py cannot be imported:
torch_geometric, cv2, svgpathtools are absent); their line ranges are asserted and none of their text is copied.  The three
methods are bound to a bare object; `np` and `random` resolve to the real modules, so the GLOBAL generators are consumed
exactly as the dataset's `__getitem__` consumes them.

Inputs (`augment_util.CASES`): small synthetic items whose float64 values are exactly representable in fp32 — what a
device batch can hold — with a one-node proposal, proposals of more than 64 nodes, and at least one node per proposal.
Stored per case: the inputs; per case and seed (both generators seeded with it): the reference's float64 outputs (`pos`,
`bbox` from update_bbox, `gt_bbox`, `bbox_targets`) and the next `np.random.random()` / `random.random()` after the call.
"""
import ast
import json
import os
import random
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import augment_util as au  # noqa: E402


def reference_root():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    root = args[0] if args else os.environ.get("YOLAT_REFERENCE")
    if not root or not os.path.isdir(root):
        raise SystemExit("usage: make_golden_augment.py <reference checkout> [--time]")
    return root


def reference_functions(root):
    """(me, update_bbox): an object carrying the reference's random_transfer / __transform__ / __transform_bbox__ as bound
    methods, and the nested update_bbox of __getitem__."""
    path = os.path.join(root, "Datasets", "graph_dict3.py")
    tree = ast.parse(open(path).read())
    ds_cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SESYDFloorPlan")

    def method(name, lines):
        fn = next(n for n in ds_cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
        assert (fn.lineno, fn.end_lineno) == lines, (name, fn.lineno, fn.end_lineno)
        return fn
    fns = [method("__transform__", (236, 258)), method("__transform_bbox__", (260, 281)),
           method("random_transfer", (283, 298))]
    getitem = next(n for n in ds_cls.body if isinstance(n, ast.FunctionDef) and n.name == "__getitem__")
    ub = next(n for n in getitem.body if isinstance(n, ast.FunctionDef) and n.name == "update_bbox")
    assert (ub.lineno, ub.end_lineno) == (934, 955), (ub.lineno, ub.end_lineno)      # its call: :959
    ns = {"np": np, "random": random}
    exec(compile(ast.Module(body=fns + [ub], type_ignores=[]), path, "exec"), ns)
    me = types.SimpleNamespace()
    for fn in fns:
        setattr(me, fn.name, types.MethodType(ns[fn.name], me))
    return me, ns["update_bbox"]


def run_reference(me, update_bbox, inp, seed):
    """what __getitem__ does under data_aug (:957-959), on copies (the reference edits its arguments in place)"""
    np.random.seed(seed)
    random.seed(seed)
    pos, bbox, gt_bbox, bbox_targets = me.random_transfer(inp["pos"].copy(), inp["bbox"].copy(), inp["gt_bbox"].copy(),
                                                          inp["bbox_targets"].copy())
    bbox = update_bbox(pos, inp["bbox_idx"])
    return {"pos": pos, "bbox": bbox, "gt_bbox": gt_bbox, "bbox_targets": bbox_targets,
            "next_np": np.float64(np.random.random()), "next_py": np.float64(random.random())}


def main():
    root = reference_root()
    me, update_bbox = reference_functions(root)
    out = {}
    for name in au.CASES:
        inp = au.case_inputs(name)
        for k, v in inp.items():
            if v.dtype == np.float64:
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v), (name, k)
            out["%s/%s" % (name, k)] = v
        assert np.bincount(inp["bbox_idx"], minlength=inp["bbox"].shape[0]).min() >= 1
        for seed in au.SEEDS:
            res = run_reference(me, update_bbox, inp, seed)
            assert res["bbox"].shape == inp["bbox"].shape
            for k, v in res.items():
                out["%s/s%d/%s" % (name, seed, k)] = np.asarray(v, dtype=np.float64)
        print(name, "nodes:", inp["pos"].shape[0], "proposals:", inp["bbox"].shape[0],
              "largest:", int(np.bincount(inp["bbox_idx"]).max()))
    out["provenance"] = np.array("outputs of the reference's own SESYDFloorPlan.random_transfer + update_bbox "
                                 "(Datasets/graph_dict3.py:236-298, 934-959, compiled from its source text), float64")
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    if "--time" in sys.argv:
        time_reference(me, update_bbox)


def time_reference(me, update_bbox):
    """the reference's per-item cost of random_transfer + update_bbox at the item shapes of the cfg-3 / cfg-4 batches,
    single-threaded Python as a DataLoader worker runs it -> tests/golden/reference_timings_augment.json"""
    res = {"host": {"cpus": os.cpu_count(), "threads_used": 1,
                    "note": "build container; single-threaded Python as the reference runs it"},
           "reference": "Datasets/graph_dict3.py:283-298 (random_transfer) + :934-959 (update_bbox)"}
    for tag, (P, lo, hi, B) in au.TIMING_SHAPES.items():
        inp = au.synth_inputs(P, lo, hi, seed=17)
        ts = []
        for rep in range(5):
            args = [inp[k].copy() for k in ("pos", "bbox", "gt_bbox", "bbox_targets")]
            t0 = time.perf_counter()
            pos, _, _, _ = me.random_transfer(*args)
            t1 = time.perf_counter()
            update_bbox(pos, inp["bbox_idx"])
            t2 = time.perf_counter()
            ts.append((t2 - t0, t1 - t0, t2 - t1))
        ts.sort()
        med = ts[len(ts) // 2]
        res[tag] = {"proposals_per_item": P, "nodes_per_item": int(inp["pos"].shape[0]), "items_per_batch": B,
                    "seconds_per_item": med[0], "seconds_random_transfer": med[1], "seconds_update_bbox": med[2],
                    "seconds_per_batch": med[0] * B}
    path = os.path.join(HERE, "reference_timings_augment.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
