"""float64 reference helpers for the bf16-STORAGE eval forward of a LEAKY model (act = leakyrelu / prelu: csrc/act.hip,
the ACT instantiation of k_hfusion_rows8 in fusion_h8.hip, k_hgemm_act and the materialising fusion route in
bf16_eval.hip).  The stage model of tests/bf16_eval_ref.py extended by the activation; CPU or GPU tensors alike, torch
only, no import of the extension (tests/test_bf16_act_ref_host.py checks every claim made here on the CPU,
tests/test_gpu_bf16_act_stages.py holds the kernels to it).

Model of a stage
  * (val, delta) = the pre-activation value and envelope of bf16_eval_ref.stage_ref with relu=False: exact products of the
    bf16 operand values summed in float64, the epilogue form in float64, delta the fp32 accumulation + epilogue bound;
  * want = act(val), act(y) = y > 0 ? y : a y, the slope `a` being the fp32 number the kernel reads, widened;
  * envelope = max(1, |a|) delta + 2^-24 |a val|: act is continuous and piecewise linear with slopes 1 and a, hence
    max(1, |a|)-Lipschitz — also across the kink, where the fp32 value and the float64 one may take different branches —
    and the kernel's a * y is one more fp32 product, rounded once.  Derived, not measured;
  * the per-proposal maximum is taken over ACTIVATED rows (for a < 0 the activation is not monotone: the maximum of the
    activated rows is not the activation of the maximum), empty proposals are 0; a pooled element is allowed the largest
    envelope among its proposal's rows (max is 1-Lipschitz);
  * a bf16 output gets bf16_ref.store_envelope(want, envelope): the activation is applied in fp32 BEFORE the one rounding.
"""
import torch

import bf16_eval_ref as er
from bf16_ref import EPS32, bf

SLOPES = (0.2, -0.3, 1.4, 0.0)


def slope64(a):
    """the fp32 number a kernel reads for the Python float `a`, as float64"""
    return float(torch.tensor(a, dtype=torch.float32).double())


def act64(val, a):
    return torch.where(val > 0, val, a * val)


def act_envelope(val, delta, a):
    return max(1.0, abs(a)) * delta + EPS32 * (a * val).abs()


def stage_act_ref(a64, w64, form, b, s, t, a):
    """(want, envelope, val) [M,Nout] float64 of act(epilogue(a64 . w64^T))"""
    val, delta = er.stage_ref(a64, w64, form, b, s, t, relu=False)
    return act64(val, a), act_envelope(val, delta, a), val


def fusion_pool_act_ref(feats, w_bits, form, b, s, t, seg, P, a, chunk=16384):
    """pooled (want, tol, act_of_max) [P,F]: the per-proposal amax of the activated rows (empty proposals 0) with its
    envelope, and act(amax of the PRE-activation rows) — what a kernel that activates after the maximum would give"""
    F = w_bits.shape[0]
    dev = feats.device
    neg = float("-inf")
    want = torch.full((P, F), neg, dtype=torch.float64, device=dev)
    pre = torch.full((P, F), neg, dtype=torch.float64, device=dev)
    tol = torch.zeros(P, F, dtype=torch.float64, device=dev)
    w64 = er.widen(w_bits)
    for r0 in range(0, feats.shape[0], chunk):
        v, e, val = stage_act_ref(er.widen(feats[r0:r0 + chunk]), w64, form, b, s, t, a)
        sg = seg[r0:r0 + chunk]
        want.index_reduce_(0, sg, v, "amax", include_self=True)
        pre.index_reduce_(0, sg, val, "amax", include_self=True)
        tol.index_reduce_(0, sg, e, "amax", include_self=True)
    has = (torch.bincount(seg, minlength=P) > 0)[:, None]
    zero = torch.zeros_like(want)
    return torch.where(has, want, zero), tol, torch.where(has, act64(pre, a), zero)


def super_act_ref(S32, w_bits, form, b, s, t, a):
    """(want, envelope) of fusion_block_super: fp32 rows rounded to nearest even while loading"""
    want, env, _ = stage_act_ref(bf(S32), er.widen(w_bits), form, b, s, t, a)
    return want, env


def exercise(want, act_of_max, seg, P):
    """(share of negative pooled entries, share of entries of the proposals with >= 2 rows that differ from
    act(max pre), number of such proposals) — computed on the REFERENCE: do the inputs reach what the signed pooling is for?"""
    multi = torch.bincount(seg, minlength=P) >= 2
    neg = float((want < 0).double().mean())
    n = int(multi.sum())
    differ = float((want[multi] != act_of_max[multi]).double().mean()) if n else 0.0
    return neg, differ, n


# ---------------------------------------------------------------------------------------------
# fp32 emulation (host test: the envelope accepts it, and rejects the wrong kernels)
# ---------------------------------------------------------------------------------------------
def emulate_act(val32, a):
    """the kernels' literal fp32 activation"""
    a32 = torch.tensor(a, dtype=torch.float32)
    return torch.where(val32 > 0, val32, a32 * val32)


def emulate_pool_act(act32, seg, P):
    out = torch.full((P, act32.shape[1]), float("-inf"))
    out.index_reduce_(0, seg, act32, "amax", include_self=True)
    has = (torch.bincount(seg, minlength=P) > 0)[:, None]
    return torch.where(has, out, torch.zeros_like(out))


def fusion_act_inputs(lay, D, F):
    """the inputs of one fusion-pair case (bf16_eval_ref.fusion_inputs: bf16 activations >= 0, tie proposals, a quarter of
    the scales negative, s = +-0 columns, closed columns t = -50), seeded by the shape alone so that the host test examines
    exactly what the GPU test runs"""
    return er.fusion_inputs(lay, D, F, 31 * lay.N + 7 * D + F)
