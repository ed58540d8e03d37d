#!/usr/bin/env python
"""A/B timing of the fp32 eval forward: norm = batch against norm = layer / instance from this tree, and of the fusion launch
alone at the cfg-2 shapes: the fused row-norm kernel, the materialising route and the BatchNorm launch.

    python tools/rownorm_ab.py --out profiles/rownorm_ab.json [--runs 3] [--cfgs 2,5]

Every run is a fresh child process (this file with --child) that builds the cfg's model from the seeded fill of
tests/golden_util.py, stages the batch on the device once, warms up, and times K forwards between two device events (three
windows; the median and the spread are kept).  The children alternate batch / layer / layer_fused / instance, `--runs` times
(layer: the route the forward picks by the node count; layer_fused: YOLAT_RN_FUSED=1, the fused kernel whatever the count).
Each child also lists the stages of one profiled forward and times the three fusion launches on its cfg-2 batch, again
interleaved; one more child sweeps the three launches over the node count (25 nodes per proposal) — where the routes cross.
Needs the GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _window(fn, steps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps


def fusion_alone(yv, torch, data, steps=300):
    """us per launch of the three fusion launches on the batch's proposal layout (N x 128 -> 1024, pooled to P rows)."""
    from yolat_vectorgraphicsrecognition_amd import ops
    lib, check = yv._lib.lib, yv._lib.check
    g = torch.Generator().manual_seed(5)
    N, P, D, F = data.x.shape[0], data.bbox.shape[0], 128, 1024
    A = torch.relu(torch.randn(N, D, generator=g)).cuda()
    S = torch.randn(P, D, generator=g).cuda()
    W, Ws = (torch.randn(F, D, generator=g) / D ** 0.5).cuda(), (torch.randn(F, D, generator=g) / D ** 0.5).cuda()
    b, bs = (torch.randn(F, generator=g) * 0.1).cuda(), (torch.randn(F, generator=g) * 0.1).cuda()
    ga, be = (torch.rand(F, generator=g) + 0.5).cuda(), (torch.randn(F, generator=g) * 0.3).cuda()
    seg = data.bbox_idx.int().cuda()
    ZW = 2 * (F + D)
    Z = torch.zeros(P, ZW, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    cen = [ops.rownorm_center(W, b), ops.rownorm_center(Ws, bs)]
    cs = [ops.split_bf16x3(c[0]) for c in cen]
    ps = [ops.split_bf16x3(W), ops.split_bf16x3(Ws)]
    work = torch.empty(int(lib.yolat_fusion_pair_eval_rn_work_elems(N, F)), device="cuda")
    p = lambda t: t.data_ptr()

    def fused():
        check(lib.yolat_fusion_pair_eval_x6_rn(p(A), D, N, D, p(cs[0][0]), p(cs[0][1]), p(cs[0][2]), p(cen[0][1]), F, p(ga), p(be),
                                               p(seg), p(Z), ZW, p(S), D, P, p(cs[1][0]), p(cs[1][1]), p(cs[1][2]), p(cen[1][1]),
                                               p(ga), p(be), p(Z[:, F + D:]), ZW, 1e-5, st), "x6_rn")

    def generic():
        check(lib.yolat_fusion_pair_eval_rn(p(A), D, N, D, p(W), p(b), F, p(ga), p(be), p(seg), p(Z), ZW, p(S), D, P, p(Ws), p(bs),
                                            p(ga), p(be), p(Z[:, F + D:]), ZW, 1e-5, p(work), st), "rn")

    def batchnorm():
        check(lib.yolat_fusion_pair_eval_x6(p(A), D, N, D, p(ps[0][0]), p(ps[0][1]), p(ps[0][2]), p(b), F, p(seg), p(Z), ZW, p(S), D,
                                            P, p(ps[1][0]), p(ps[1][1]), p(ps[1][2]), p(bs), p(Z[:, F + D:]), ZW, st), "x6")
    legs = {"rownorm_fused": fused, "rownorm_generic": generic, "batchnorm_x6": batchnorm}
    for fn in legs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(3):
        for k, fn in legs.items():
            out[k].append(_window(fn, steps, torch))
    return {"N": N, "P": P, "D": D, "F": F, "steps_per_window": steps, "us_per_launch": {k: sorted(v) for k, v in out.items()}}


SWEEP_N = (1250, 2500, 5000, 7500, 10000, 15000, 20000, 40000, 80000, 200000)


def sweep(yv, torch):
    class Batch(object):
        pass
    out = {}
    for N in SWEEP_N:
        d, P = Batch(), N // 25
        d.x, d.bbox, d.bbox_idx = torch.zeros(N, 5), torch.zeros(P, 4), torch.arange(N) // 25
        r = fusion_alone(yv, torch, d, steps=200 if N <= 20000 else 40)
        out[str(N)] = {k: v[1] for k, v in r["us_per_launch"].items()}
    return out


def child(norm, cfgs, steps):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import ctypes
    import torch
    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv
    assert torch.cuda.is_available(), "needs the GPU"
    if norm == "sweep":
        print("RN_AB " + json.dumps(sweep(yv, torch)))
        return
    if norm == "layer_fused":
        os.environ["YOLAT_RN_FUSED"] = "1"
        norm = "layer"
    out = {}
    for cfg in cfgs:
        data, slices, optkw, _ = yv.config(cfg)
        model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**dict(optkw, norm=norm))), 3).cuda().eval()
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
        if cfg == "2":
            rec["fusion_alone"] = fusion_alone(yv, torch, data)
        out[cfg] = rec
    print("RN_AB " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cfgs", default="2,5")
    ap.add_argument("--child", default=None, metavar="NORM")
    a = ap.parse_args()
    cfgs = a.cfgs.split(",")
    steps = {c: (400 if c in ("1", "2") else 60) for c in cfgs}
    if a.child:
        return child(a.child, cfgs, steps)
    legs = ("batch", "layer", "layer_fused", "instance")
    runs = {name: [] for name in legs}

    def run_child(name):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cfgs", a.cfgs, "--child", name],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("RN_AB ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout)
            raise SystemExit("leg %s failed (rc %d)" % (name, p.returncode))
        return json.loads(line[0][6:])
    for _ in range(a.runs):
        for name in legs:
            runs[name].append(run_child(name))
            print(name, {c: runs[name][-1][c]["us_per_forward"] for c in cfgs}, flush=True)
    res = {"what": "fp32 eval forward, device-event time per forward (us): median of 3 windows per run, runs interleaved; "
                   "fusion_alone: the fusion launch by itself at the cfg-2 batch, us per launch, 3 windows per run",
           "steps_per_window": steps, "legs": {}, "fusion_alone_cfg2": {}}
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
        if "2" in cfgs:
            res["fusion_alone_cfg2"][name + "_child"] = [r["2"]["fusion_alone"] for r in runs[name]]
    res["fusion_alone_sweep_median_us"] = run_child("sweep")
    print(json.dumps(res["fusion_alone_sweep_median_us"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {c: v[c]["median_us_per_run"] for c in v} for k, v in res["legs"].items()}))
    if "2" in cfgs:
        print(json.dumps({k: [r["us_per_launch"] for r in v] for k, v in res["fusion_alone_cfg2"].items()}))


if __name__ == "__main__":
    main()
