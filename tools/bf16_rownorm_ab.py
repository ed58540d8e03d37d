#!/usr/bin/env python
"""Timing and numerics of the bf16-storage eval forward of a --norm layer / instance model
(set_eval_precision("bf16", row_norm=True); csrc/fusion_h8_rn.hip).

    python tools/bf16_rownorm_ab.py --out profiles/bf16_rownorm_timing.json [--runs 3] [--cfgs 2,5] [--parent DIR]
    python tools/bf16_rownorm_ab.py --contract profiles/bf16_rownorm_contract.txt

Timing: every run is a fresh child process (this file with --child LEG) that builds the cfg's model from the seeded fill of
tests/golden_util.py, stages the batch on the device once, warms up (20 forwards), and times K forwards between two device
events (three windows; the median and the spread are kept).  The children alternate over the legs, `--runs` times:
    batch_bf16            norm = batch, bf16 storage (the forward the row-norm one is compared with)
    layer_bf16_fused      norm = layer, bf16 storage, the fused fusion kernel (YOLAT_RN_FUSED=1)
    layer_bf16_mat        the same model on the materialising route (YOLAT_RN_FUSED=0)
    instance_bf16_fused   norm = instance (gamma NULL)
    layer_fp32            norm = layer, the fp32 forward of this tree (the route its node count picks)
    layer_fp32_parent     the same forward from the checkout given with --parent (a built tree of the parent commit), on the
                          same box in the same alternation
Each child also lists the stages of one profiled forward.
Contract: the logit gap of the bf16 forward against the fp32 forward of the same model — max and rms relative to the logits'
scale / rms, arg-max agreement — on the graphs of tests/test_gpu_bf16_rownorm_model.py (both routes) and on the cfg-2 and
cfg-5 random graphs (two weight seeds).  Needs the GPU: there is no CPU fall-back."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"batch_bf16": ("batch", "bf16", None), "layer_bf16_fused": ("layer", "bf16", "1"), "layer_bf16_mat": ("layer", "bf16", "0"),
        "instance_bf16_fused": ("instance", "bf16", "1"), "layer_fp32": ("layer", "fp32", None),
        "layer_fp32_parent": ("layer", "fp32", None)}


def _window(fn, steps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps


def _imports(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv
    assert torch.cuda.is_available(), "needs the GPU"
    assert os.path.dirname(os.path.dirname(os.path.abspath(yv.__file__))) == os.path.abspath(root), yv.__file__
    return torch, gu, yv


def child(leg, cfgs, steps, root):
    import ctypes
    norm, precision, fused = LEGS[leg]
    if fused is not None:
        os.environ["YOLAT_RN_FUSED"] = fused
    torch, gu, yv = _imports(root)
    out = {}
    for cfg in cfgs:
        data, slices, optkw, _ = yv.config(cfg)
        model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**dict(optkw, norm=norm))), 3).cuda().eval()
        if precision == "bf16":
            model.set_eval_precision("bf16", **({"row_norm": True} if norm != "batch" else {}))
        d = yv.Data(x=data.x.cuda().float(), pos=data.pos)
        for k in ("edge", "e_attr", "bbox_idx", "bbox"):
            d[k] = data[k].cuda()
        with torch.no_grad():
            for _ in range(20):
                logits = model(d, None)[0]
            torch.cuda.synchronize()
            wins = [_window(lambda: model(d, None), steps[cfg], torch) for _ in range(3)]
        rec = {"us_per_forward": sorted(wins), "logits_abs_sum": float(logits.double().abs().sum()),
               "N": int(data.x.shape[0]), "P": int(data.bbox.shape[0])}
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
    print("BRN_AB " + json.dumps(out))


def contract(path):
    torch, gu, yv = _imports(HERE)
    import test_gpu_bf16_rownorm_model as tm
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def measure(tag, model, run):
        with torch.no_grad():
            want = run(model).clone()
            model.set_eval_precision("bf16", row_norm=True)
            got = run(model).clone()
        mx, rms, agree = tm.gap(got, want)
        say("%-46s max %.3e  rms %.3e  arg-max agreement %.4f  (P = %d)" % (tag, mx, rms, agree, got.shape[0]))
        flip = got.argmax(1) != want.argmax(1)
        if bool(flip.any()):
            top2 = want[flip].topk(2, dim=1).values
            g = (top2[:, 0] - top2[:, 1]) / want.abs().max()
            say("    flips: %d of %d; fp32 top-2 gap of the flipped rows / scale: median %.2e  max %.2e"
                % (int(flip.sum()), got.shape[0], float(g.median()), float(g.max())))
        return mx

    say("bf16-storage eval forward of a row-norm model against the fp32 HIP forward of the same model: max |gap| / max |logit|,")
    say("rms gap / rms logit, arg-max agreement.  Test graphs: tests/test_gpu_bf16_rownorm_model.py (seed 31); cfg: yv.config.")
    worst = 0.0
    for norm, shape, route in tm.CASES:
        os.environ["YOLAT_RN_FUSED"] = "1" if route == "fused" else "0"
        d = tm.graph(shape)
        worst = max(worst, measure("test graph %-5s %-8s %-7s" % (shape, norm, route), tm.build(yv, norm, shape), lambda m: m(d, None)[0]))
    say("largest max over the test graphs: %.3e" % worst)
    os.environ.pop("YOLAT_RN_FUSED")
    for cfg in ("2", "5"):
        data, slices, optkw, _ = yv.config(cfg)
        for k in ("x", "edge", "e_attr", "bbox_idx", "bbox"):
            data[k] = data[k].cuda()
        for norm in ("layer", "instance"):
            for seed in (55, 9):
                for route in ("1", "0"):
                    os.environ["YOLAT_RN_FUSED"] = route
                    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**dict(optkw, norm=norm))), seed).cuda().eval()
                    measure("cfg %s %-8s seed %2d %s" % (cfg, norm, seed, "fused" if route == "1" else "materialise"), model,
                            lambda m: m(data, slices)[0])
    os.environ.pop("YOLAT_RN_FUSED")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cfgs", default="2,5")
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit (leg layer_fp32_parent)")
    ap.add_argument("--contract", default=None, metavar="TXT")
    ap.add_argument("--child", default=None, metavar="LEG")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    cfgs = a.cfgs.split(",")
    steps = {c: (400 if c in ("1", "2") else 60) for c in cfgs}
    if a.child:
        return child(a.child, cfgs, steps, a.root)
    if a.contract:
        return contract(a.contract)
    legs = [l for l in LEGS if l != "layer_fp32_parent" or a.parent]
    runs = {name: [] for name in legs}

    def run_child(name):
        root = a.parent if name == "layer_fp32_parent" else HERE
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cfgs", a.cfgs, "--child", name, "--root", root],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("BRN_AB ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout)
            raise SystemExit("leg %s failed (rc %d)" % (name, p.returncode))
        return json.loads(line[0][7:])
    for _ in range(a.runs):
        for name in legs:
            runs[name].append(run_child(name))
            print(name, {c: runs[name][-1][c]["us_per_forward"] for c in cfgs}, flush=True)
    res = {"what": "eval forward, device-event time per forward (us): median of 3 windows per run, runs interleaved, every run a "
                   "fresh process; 20 warm-up forwards", "steps_per_window": steps, "legs": {}}
    for name in runs:
        res["legs"][name] = {}
        for c in cfgs:
            med = [r[c]["us_per_forward"][1] for r in runs[name]]
            res["legs"][name]["cfg" + c] = {
                "N": runs[name][0][c]["N"], "P": runs[name][0][c]["P"],
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
