#!/usr/bin/env python
"""Timing of the bf16-storage eval forward of a leaky model: act = leakyrelu in bf16 against the same model in fp32 and
against the ReLU model in bf16 from this tree, and (optionally) the ReLU bf16 forward of ANOTHER tree — the parent commit,
checked out and built somewhere — with the same script, interleaved.

    python tools/bf16_act_ab.py --out profiles/bf16_act_timing.json [--parent DIR] [--runs 3] [--cfgs 2,5]

Every run is a fresh child process (this file with --child) that imports the package from one tree, builds the cfg's model
from the seeded fill of tests/golden_util.py, stages the batch on the device once, warms up, and times K forwards between
two device events (three windows, the median and the spread are kept).  The children alternate
parent-relu-bf16 / relu-bf16 / leakyrelu-bf16 / leakyrelu-fp32, `--runs` times.  The leaky bf16 child also lists the stages
of one profiled forward, so that the extra launches are listed, not guessed.  Needs the GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tree, act, precision, cfgs, steps):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import ctypes
    import torch
    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv
    assert torch.cuda.is_available(), "needs the GPU"
    out = {}
    for cfg in cfgs:
        data, slices, optkw, _ = yv.config(cfg)
        kw = dict(optkw) if act == "relu" else dict(optkw, act=act)
        model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**kw)), 3).cuda().eval()
        model.set_eval_precision(precision, **({} if act == "relu" else {"leaky_act": True}))
        d = yv.Data(x=data.x.cuda().float(), pos=data.pos)
        for k in ("edge", "e_attr", "bbox_idx", "bbox"):
            d[k] = data[k].cuda()
        with torch.no_grad():
            for _ in range(20):
                logits = model(d, None)[0]
            torch.cuda.synchronize()
            wins = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps[cfg]):
                    model(d, None)
                e1.record()
                e1.synchronize()
                wins.append(e0.elapsed_time(e1) * 1000.0 / steps[cfg])
        rec = {"us_per_forward": sorted(wins), "logits_abs_sum": float(logits.double().abs().sum())}
        lib = yv._lib.lib
        lib.yolat_profile_reset()
        lib.yolat_profile_enable(1)
        with torch.no_grad():
            model(d, None)
        torch.cuda.synchronize()
        lib.yolat_profile_enable(0)
        names = []
        for i in range(lib.yolat_profile_count()):
            buf = ctypes.create_string_buffer(160)
            ms, calls = ctypes.c_float(), ctypes.c_int()
            lib.yolat_profile_get(i, buf, 160, ctypes.byref(ms), ctypes.byref(calls), None, None)
            names.append([buf.value.decode(), calls.value, round(ms.value * 1000.0, 2)])
        rec["stages_name_calls_us"] = names
        out[cfg] = rec
    print("BF16_ACT_AB " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cfgs", default="2,5")
    ap.add_argument("--child", nargs=3, default=None, metavar=("TREE", "ACT", "PRECISION"))
    a = ap.parse_args()
    cfgs = a.cfgs.split(",")
    steps = {c: (400 if c in ("1", "2") else 60) for c in cfgs}
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], cfgs, steps)
    legs = ([("parent_relu_bf16", a.parent, "relu", "bf16")] if a.parent else []) + [
        ("relu_bf16", HERE, "relu", "bf16"), ("leakyrelu_bf16", HERE, "leakyrelu", "bf16"),
        ("leakyrelu_fp32", HERE, "leakyrelu", "fp32")]
    runs = {leg[0]: [] for leg in legs}
    for _ in range(a.runs):
        for name, tree, act, prec in legs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cfgs", a.cfgs, "--child", tree, act, prec],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("BF16_ACT_AB ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout)
                raise SystemExit("leg %s failed (rc %d)" % (name, p.returncode))
            runs[name].append(json.loads(line[0][12:]))
            print(name, {c: runs[name][-1][c]["us_per_forward"] for c in cfgs}, flush=True)
    res = {"what": "eval forward, device-event time per forward (us): median of 3 windows per run, runs interleaved; "
                   "cfg5 is configs[4]",
           "steps_per_window": steps, "legs": {}}
    for name in runs:
        res["legs"][name] = {}
        for c in cfgs:
            med = [r[c]["us_per_forward"][1] for r in runs[name]]
            res["legs"][name]["cfg" + c] = {
                "median_us_per_run": med, "min_us": min(med), "max_us": max(med),
                "windows_us": [r[c]["us_per_forward"] for r in runs[name]],
                "logits_abs_sum": runs[name][0][c]["logits_abs_sum"],
                "stages_name_calls_us": runs[name][0][c].get("stages_name_calls_us")}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {c: v[c]["median_us_per_run"] for c in v} for k, v in res["legs"].items()}))


if __name__ == "__main__":
    main()
