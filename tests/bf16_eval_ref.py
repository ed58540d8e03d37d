"""float64 reference helpers for the dense stages of the bf16-STORAGE eval forward (csrc/bf16_eval.hip, fusion_h8.hip):
the fusion pair on its five routes, the pooling prologue, the node side of the layers > 0 and the classifier's GEMM.  CPU
or GPU tensors alike: torch only, no import of the extension (tests/test_bf16_eval_ref_host.py checks every claim made
here on the CPU; tests/test_gpu_bf16_eval_stages.py holds the kernels to it).  Built on tests/bf16_ref.py.

Model of a stage
  * operands are the bf16 values the kernel multiplies: the weight BITS the test hands to the kernel widened to float64
    (never re-derived from an fp32 weight), activations stored as bf16 widened, activations given as fp32 rounded to
    nearest even (bf16_ref.bf);
  * products exact, summed in float64 (`dot`); `mag` = |a| . |w| is the magnitude sum of the same products;
  * the epilogue in float64, as the code computes it (FORMS):
      fold   relu(dot + t)                  k_hfusion_rows8: the BatchNorm scale is inside the weight bits, t = s b + t
      rows   relu(dot s + (b s + t))        k_hfusion_rows (hgemm_rows' pooling epilogue)
      tile   relu((dot + b) s + t)          hgemm_tile's wave_epilogue: k_hgemm, k_hgemm_two, k_hgemm_node3, the super block
  * the per-proposal max is index_reduce_(amax) with empty proposals at 0 (the activations are >= 0);
  * the pooling prologue is the exact max of the widened bf16 values (0 for an empty proposal) and sum / max(cnt, 1).

Envelope, per element, nothing scaled by a tensor maximum:
    delta = |s| dot_delta(mag, K) + 4 2^-24 (|dot s| + |b s| + |t|)          (s = 1, b = 0 where the form has none)
  dot_delta (bf16_ref.py) is the fp32 accumulation bound of the K products; the second term covers the epilogue's at most
  four fp32 roundings (bias add or bias product, the fma, ReLU is exact), each of a value no larger than the bracket.  (In the
  fold form the shift is the accumulators' initial value and is rounded with every MFMA step, not once: where the
  products are tiny beside the shift that form comes closest to the envelope, 0.84 of it as measured.)  ReLU
  and max are 1-Lipschitz: a pooled element is allowed the largest delta among its proposal's rows, and no element is left
  out.  A bf16 output gets store_envelope(want, delta).  The mean of cnt rows summed one by one in fp32 and divided once:
  (cnt + 2) 2^-24 sum|v| / max(cnt, 1).  Prologue maxima and the zero block are bit-equal.
"""
import numpy as np
import torch

import segmax_layouts as sl
from bf16_ref import EPS32, bf, dot_delta

FORMS = ("fold", "rows", "tile")


def widen(t):
    """float64 image of a bfloat16 tensor (exact)"""
    assert t.dtype == torch.bfloat16, t.dtype
    return t.double()


def gemm_ref(a64, w64):
    """(dot, mag) = (a . w^T, |a| . |w|^T) in float64; a64 [M,K], w64 [Nout,K] hold bf16 values"""
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def _vec(v, like, fill):
    if v is None:
        return torch.full((like.shape[1],), fill, dtype=torch.float64, device=like.device)
    return v.to(like.device).double()


def epilogue_ref(dot, mag, K, form, b=None, s=None, t=None, relu=True):
    """(want, delta) [M,Nout] float64 of one epilogue form on a K-long dot product"""
    assert form in FORMS
    b, s, t = _vec(b, dot, 0.0), _vec(s, dot, 1.0), _vec(t, dot, 0.0)
    if form == "fold":
        val = dot + t
    elif form == "rows":
        val = dot * s + (b * s + t)
    else:
        val = (dot + b) * s + t
    delta = s.abs() * dot_delta(mag, K) + 4.0 * EPS32 * ((dot * s).abs() + (b * s).abs() + t.abs())
    return (torch.relu(val) if relu else val), delta.expand_as(val)


def stage_ref(a64, w64, form, b=None, s=None, t=None, relu=True):
    dot, mag = gemm_ref(a64, w64)
    return epilogue_ref(dot, mag, a64.shape[1], form, b, s, t, relu)


def fusion_pool_ref(feats, w_bits, form, b, s, t, seg, P, chunk=16384):
    """pooled (want, tol) of the node problem, in row chunks (a 66 000 x 1024 float64 matrix need not exist at once)"""
    F = w_bits.shape[0]
    want = torch.zeros(P, F, dtype=torch.float64, device=feats.device)
    tol = torch.zeros_like(want)
    w64 = widen(w_bits)
    for r0 in range(0, feats.shape[0], chunk):
        val, delta = stage_ref(widen(feats[r0:r0 + chunk]), w64, form, b, s, t)
        want.index_reduce_(0, seg[r0:r0 + chunk], val, "amax", include_self=True)
        tol.index_reduce_(0, seg[r0:r0 + chunk], delta, "amax", include_self=True)
    return want, tol


def super_ref(S32, w_bits, form, b, s, t):
    """(want, delta) of fusion_block_super: fp32 rows rounded to nearest even while loading"""
    return stage_ref(bf(S32), widen(w_bits), form, b, s, t)


def pool_prepare_ref(feats, fsup, seg, P):
    """(max [P,D] of the feats rows (0: empty), mean [P,D] of the fsup rows, tolerance of the mean); feats / fsup bf16"""
    D = feats.shape[1]
    f64, s64 = widen(feats), widen(fsup)
    cnt = torch.bincount(seg, minlength=P).double()
    mx = torch.full((P, D), float("-inf"), dtype=torch.float64, device=feats.device)
    mx.index_reduce_(0, seg, f64, "amax", include_self=True)
    mx = torch.where((cnt > 0)[:, None], mx, torch.zeros_like(mx))
    sm = torch.zeros(P, D, dtype=torch.float64, device=feats.device).index_add_(0, seg, s64)
    mag = torch.zeros(P, D, dtype=torch.float64, device=feats.device).index_add_(0, seg, s64.abs())
    den = cnt.clamp_min(1.0)[:, None]
    return mx, sm / den, (cnt[:, None] + 2.0) * EPS32 * mag / den


# ---------------------------------------------------------------------------------------------
# inputs (the recipe of test_gpu_fusion_pool.py::test_fusion_pair_eval_vs_fp64, activations drawn AS bf16)
# ---------------------------------------------------------------------------------------------
def activations(lay, D, tg, ties=True):
    """[N,D] bfloat16 >= 0, tie proposals filled with copies of their first row"""
    A = (torch.relu(torch.randn(lay.N, D, generator=tg)) + 0.3 * torch.rand(1, D, generator=tg)).to(torch.bfloat16)
    st = sl.starts(lay)
    for p in (sl.tie_proposals(lay) if ties else ()):
        A[st[p]:st[p] + lay.sizes[p]] = A[st[p]].clone()
    return A


def bn_vectors(F, tg, negative=True):
    """(b, s, t) fp32 [F]: about a quarter of the scales negative, s = +0 / -0.0 columns with t > 0, closed columns"""
    b = torch.randn(F, generator=tg) * 0.1
    s = torch.rand(F, generator=tg) - 0.3 if negative else torch.rand(F, generator=tg) + 0.5
    t = torch.randn(F, generator=tg) * 0.2
    s[0::16], s[1::16] = 0.0, -0.0
    t[0::16], t[1::16] = 0.4, 0.7
    t[2::16] = -50.0
    return b, s, t


def fusion_inputs(lay, D, F, seed, ties=True):
    """feats [N,D] bf16, S [P,D] fp32 (the super block's input), both weight forms of both blocks:
    W / Ws bf16 bits of the fp32 weights with (b, s, t) / (bs, ss, ts); Wfold = bf16(s W) with tfold = s b + t (fp32)"""
    tg = torch.Generator().manual_seed(seed)
    inp = dict(feats=activations(lay, D, tg, ties), S=torch.randn(lay.P, D, generator=tg))
    for k, neg in (("", True), ("s", False)):
        W32 = torch.randn(F, D, generator=tg) / D ** 0.5
        b, s, t = bn_vectors(F, tg, neg)
        inp["W" + k], inp["b" + k], inp["s" + k], inp["t" + k] = W32.to(torch.bfloat16), b, s, t
        inp["Wfold" + k], inp["tfold" + k] = (s[:, None] * W32).to(torch.bfloat16), s * b + t
    return inp


# ---------------------------------------------------------------------------------------------
# fp32 emulation of a stage (host test: the envelope accepts it and rejects the wrong kernels)
# ---------------------------------------------------------------------------------------------
def emulate_stage(a_bf, w_bits, form, b=None, s=None, t=None, relu=True, acc=None):
    """The kernel's arithmetic in fp32 on the CPU: bf16 operands widened to fp32, fp32 matmul, fp32 epilogue.  a_bf:
    bfloat16 rows; acc: a ready fp32 accumulator instead of the product (the mutations build their own)."""
    if acc is None:
        acc = a_bf.float() @ w_bits.float().t()
    one, zero = torch.ones(acc.shape[1]), torch.zeros(acc.shape[1])
    b, s, t = (zero if b is None else b.float()), (one if s is None else s.float()), (zero if t is None else t.float())
    if form == "fold":
        val = acc + t
    elif form == "rows":
        val = acc * s + (b * s + t)
    else:
        val = (acc + b) * s + t
    return torch.relu(val) if relu else val


def emulate_pool(val32, seg, P):
    out = torch.zeros(P, val32.shape[1])
    return out.index_reduce_(0, seg, val32, "amax", include_self=True)


def worst(name, got, want, tol):
    """prints and returns the worst error / tolerance and the number of elements outside (NaN counts as outside)"""
    err = (got.double() - want).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print("ratio %-44s %.3f" % (name, ratio))
    return ratio, int(bad.sum())


def plan_h8(N, F, force=0):
    """(groups, ng) of the N-row problem as yl_hfusion_rows8 plans it (fusion_h8.hip `split`)"""
    tn, tm = F // 64, -(-N // 256)
    best, groups, g = None, 1, 1
    while g <= tn:
        cost = -(-(tm * g) // 512) * (2 + -(-tn // g))
        if best is None or cost < best:
            best, groups = cost, g
        g *= 2
    if force > 0:
        groups = force
    ng = -(-tn // groups)
    return -(-tn // ng), ng


def plan_rows(N, F, force=0):
    """(groups, ng) of the k_hfusion_rows routes (bf16_eval.hip)"""
    tn, tm = -(-F // 64), -(-N // 64)
    groups = 4
    while tm * groups < 1024 and groups < tn:
        groups *= 2
    if force > 0:
        groups = force
    groups = min(groups, tn)
    ng = -(-tn // groups)
    return -(-tn // ng), ng


def seg_tensor(lay):
    return torch.from_numpy(np.ascontiguousarray(lay.bbox_idx))
