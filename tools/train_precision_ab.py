"""A/B of the training precisions on one box: Trainer.step at cfg 3 and cfg 5 in fp32 / bf16 / bf16_dense, 20 warm-up and
50 timed steps each (device time between two events around the timed steps, divided by the step count), same model
initialisation and batch per config.  Prints one JSON line per (config, precision) and a summary line with the ratio
bf16_dense / bf16.

    python tools/train_precision_ab.py [--configs 3,5] [--warmup 20] [--steps 50] [--only PREC]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--precisions", default="fp32,bf16,bf16_dense")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    import torch
    import golden_util as gu
    import yolat_vectorgraphicsrecognition_amd as yv
    torch.cuda.set_device(0)
    out = {}
    for cfg in args.configs.split(","):
        data, slices, optkw, _ = yv.config(cfg)
        for k in ("x", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
            data[k] = data[k].cuda()
        for prec in args.precisions.split(","):
            opt = yv.Opt(**optkw)
            model = gu.fill_state_(yv.SparseCADGCN(opt), 21).cuda()
            tr = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5, precision=prec)
            for _ in range(args.warmup):
                loss = tr.step(data, slices)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                loss = tr.step(data, slices)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            rec = {"config": cfg, "precision": prec, "ms_per_step": round(ms, 4), "plan_steps": tr.plan_steps,
                   "steps": args.warmup + args.steps, "final_loss": float(loss)}
            out[(cfg, prec)] = ms
            print(json.dumps(rec), flush=True)
            del tr, model
            torch.cuda.empty_cache()
        if (cfg, "bf16") in out and (cfg, "bf16_dense") in out:
            print(json.dumps({"config": cfg, "bf16_dense_over_bf16": round(out[(cfg, "bf16_dense")] / out[(cfg, "bf16")], 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
