"""The measurement of tools/exp/bf16_contract.py repeated for leaky models: the bf16-storage eval forward against the fp32
HIP forward of the same model on the BASELINE configurations, for act = leakyrelu and for act = prelu with every slope at
-0.3 (not monotone: the signed pooling's case) — max / rms error of the logits relative to their scale and arg-max
agreement, on the forward's default route.   usage: python tools/exp/bf16_act_contract.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu
import yolat_vectorgraphicsrecognition_amd as yv


def rel(got, want):
    got, want = got.double(), want.double()
    sc = float(want.abs().max())
    return (float((got - want).abs().max()) / sc, float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()),
            float((got.argmax(1) == want.argmax(1)).double().mean()))


for cfg in ("1", "2", "4", "5"):
    data, slices, optkw, _ = yv.config(cfg)
    for k in ("x", "edge", "e_attr", "bbox_idx", "bbox"):
        data[k] = data[k].cuda()
    for variant, act, slope in (("leakyrelu", "leakyrelu", None), ("prelu_neg", "prelu", -0.3)):
        for seed in (55, 9):
            model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**dict(optkw, act=act))), seed)
            if slope is not None:
                with torch.no_grad():
                    for mod in model.modules():
                        if isinstance(mod, torch.nn.PReLU):
                            mod.weight.fill_(slope)
            model = model.cuda().eval()
            with torch.no_grad():
                want = model(data, slices)[0].clone()
                model.set_eval_precision("bf16", leaky_act=True)
                got = model(data, slices)[0].clone()
            mx, rms, agree = rel(got, want)
            print("cfg %s %-9s seed %2d  max %.3e  rms %.3e  arg-max agreement %.4f" % (cfg, variant, seed, mx, rms, agree))
            flip = got.argmax(1) != want.argmax(1)
            if bool(flip.any()):
                top2 = want[flip].topk(2, dim=1).values
                gap = (top2[:, 0] - top2[:, 1]) / want.abs().max()
                print("          flips: %d of %d; fp32 top-2 gap of the flipped rows / scale: median %.2e  max %.2e"
                      % (int(flip.sum()), got.shape[0], float(gap.median()), float(gap.max())))
