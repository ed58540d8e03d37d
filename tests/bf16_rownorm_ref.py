"""float64 reference, envelope, CPU emulations and planted defects for the bf16-storage eval forward behind a ROW norm
(--norm layer / instance): the fusion pair on its two routes and the classifier's row norm (csrc/fusion_h8_rn.hip, the
row-norm branches of csrc/bf16_eval.hip).  CPU or GPU tensors alike: torch only, no import of the extension
(tests/test_bf16_rownorm_ref_host.py checks every claim made here on the CPU; tests/test_gpu_bf16_rownorm_ops.py holds the
kernels to it).  Built on tests/bf16_ref.py and tests/bf16_eval_ref.py.

Reference (rownorm_ref), on the operands the kernel actually reads — the bf16 rows widened, the weight BITS handed to the
kernel widened, the fp32 bias / gamma / beta widened:
    y = a . w^T + b,   mean = mean_c(y),   d = y - mean,   var = mean_c(d^2) (biased),   rstd = 1 / sqrt(var + eps)
    z = relu(d rstd gamma + beta)
all in float64.  The fused kernel reads the CENTRED operands (center(): Wc = W - mean over the F outputs in float64, rounded
to bf16; bc = b - mean(b), rounded to fp32), the materialising route the plain ones; each route has its own reference.

Envelope, per element, nothing scaled by a tensor maximum.  With u = 2^-24 (fp32), h = 2^-9 (bf16):
  dd     = dot_delta(|a| . |w| + |b|, K)                      fp32 accumulation of the K products and the bias (bf16_ref.py)
  e_d    bound of (deviation the kernel holds) - d:
           fused         dd + mean_c(dd) + (F + 2) u mean_c(|y| + dd).  The centred weights make the accumulator the
                         deviation up to the row mean m that the ROUNDING of Wc and bc leaves behind: the unrounded Wc has
                         column means exactly zero, so m[r] = sum_k a[r,k] mean_c(Wc_bits - Wc)[.,k] + mean(bc_fp32 - bc),
                         and with |x_bits - x| <= h |x| <= h / (1 - h) |x_bits|
                             |m[r]| <= m_w[r] = h / (1 - h) sum_k |a[r,k]| mean_c |Wc_bits[c,k]| + u mean_c |bc[c]|
                         (residual_mean_bound) — ~1e-2 of a row's standard deviation at D = 128, four orders above fp32
                         rounding.  An envelope that let it through would also let through a variance divided by F - 1
                         (defect_unbiased, 8e-3 at F = 64).  So this bound DECIDES that sweep 1 of the kernel carries
                         sum(d) and removes m: what is left is the error of that fp32 sum of F accumulators, each of
                         magnitude <= |y| + dd, and the GEMM's own error directly and through the mean.
           materialise   dd + mean_c(dd) + u (3 |y - y0| + (F + 2) mean_c |y - y0|).  yolat_rownorm_act centres on the row's
                         first element: one rounding of v = y - y0, the fp32 sum of F such terms for the mean, one rounding
                         of v - (mean - y0); the GEMM's own error enters once directly and once through the mean.
  x      = (dv + 3 (F + 2) u mean_c((|y - c| + dd)^2)) / (var + eps),   dv = 2 sqrt(var) rms_c(e_d) + mean_c(e_d^2)
                         relative error of the variance argument: Cauchy-Schwarz on mean((d + e)^2) - mean(d^2), then the fp32
                         sum of F non-negative squares in any order; the squares are those of the values the kernel holds:
                         y - y0 (c = y0) on the materialising route, the accumulators (c = 0) in the fused kernel, which
                         also forms m^2 and subtracts it (m^2 <= mean of the squares: the factor 3 covers both)
  rel    = 1 / sqrt(1 - x) - 1 + 10 u          the worse direction of (1 + -x)^-1/2, then sqrtf (1 ulp = 2 u), the division
                         (2.5 ulp = 5 u), the multiply by 1 / F and the addition of eps (u each), rounded up
  delta  = |gamma| rstd (e_d (1 + rel) + |d| rel) + 4 u (|d rstd gamma| + |beta|)
                         the deviation error and the rstd error pushed through rstd gamma, then the product, the fma
ReLU and max are 1-Lipschitz: a pooled element is allowed the largest delta among its proposal's rows; an empty proposal is
exactly 0.  A bf16 output (the classifier's norm) gets bf16_ref.store_envelope(want, delta).

Emulations (fp32 on the CPU, in the kernels' arithmetic order): emulate_fused — accumulators, per-lane partial sums of d^2
over the column tiles (a lane holds column l and l + 32 of every tile), the butterfly over the 32 lanes, 1 / sqrt, fma;
emulate_rows — yolat_rownorm_act / k_rownorm_act_h: centred on the first element, lane = column mod 64, butterfly over 64.
Planted defects (each a kernel somebody could have written): defect_var_e2 — un-centred weights, a mean sweep, the variance as
E[y^2] - mean^2; defect_uncentred — un-centred weights and NO mean sweep (the accumulator taken for the deviation);
defect_unbiased — the variance divided by F - 1; defect_no_mean_sweep — the centred bf16 weights without the sum of d;
emulate_rows_h(store="truncate") — the bf16 store without rounding."""
from collections import namedtuple

import numpy as np
import torch

import segmax_layouts as sl
from bf16_ref import EPS32, bf, dot_delta, store_envelope, truncate_bf16
from bf16_eval_ref import widen

H16 = 2.0 ** -9             # unit round-off of bfloat16 (round to nearest)
EPS_NORM = 1e-5             # torch's default eps of LayerNorm / InstanceNorm1d

Case = namedtuple("Case", "layout D F norm shift zero_row")
# every fusion-pair case of tests/test_gpu_bf16_rownorm_ops.py: D in {64, 128}, F = 64 (one tile) and 1024, both norms,
# N = 1, N = 257 (the last row alone in its workgroup), a proposal over four row tiles, one-node proposals, more than FX_NP
# proposals in a tile, empty proposals, a zero row with zero bias, rows with |row mean| / std >= 100 (shift)
CASES = (
    Case("one", 128, 1024, "layer", 0.0, False),
    Case("one", 64, 64, "instance", 0.0, False),
    Case("n1", 128, 1024, "layer", 0.0, False),
    Case("n1", 64, 64, "instance", 0.0, False),
    Case("n257", 128, 1024, "layer", 0.0, True),
    Case("n257", 64, 1024, "instance", 0.0, True),
    Case("tiny_then_long", 128, 1024, "layer", 0.0, False),
    Case("tiny_then_long", 64, 64, "layer", 0.0, False),
    Case("ones300", 128, 64, "instance", 0.0, False),
    Case("empty", 128, 64, "layer", 0.0, False),
    Case("empty", 64, 1024, "instance", 0.0, False),
    Case("straddle", 128, 1024, "layer", 400.0, False),
    Case("straddle", 64, 1024, "instance", 400.0, False),
    Case("small_n33", 192, 64, "layer", 0.0, False),          # D outside {64, 128}: the materialising route whatever rn_route says
)


def case_id(c):
    return "%s-D%d-F%d-%s%s%s" % (c.layout, c.D, c.F, c.norm, "-shift" if c.shift else "", "-zero" if c.zero_row else "")


def layout(name):
    if name == "n1":
        return sl._from_sizes(name, [1])
    if name == "n257":
        # 256 + 1 rows: the last row sits alone in the second workgroup and is a proposal of its own
        return sl._from_sizes(name, [200, 56, 1], edges=(200, 256))
    if name == "ones300":
        # one node per proposal: 256 proposals in the first row tile (the first FX_NP in the LDS table, the rest direct)
        return sl._from_sizes(name, [1] * 300)
    return sl.layout(name)


def center(W32, b32):
    """(Wc bits [F,K] bfloat16, bc [F] fp32): the weight centred over its F outputs and the centred bias, in float64, each
    rounded once — what plan.rownorm_bf16_operands hands the fused kernel"""
    w = W32.double()
    b = b32.double()
    return (w - w.mean(0, keepdim=True)).to(torch.bfloat16), (b - b.mean()).float()


def inputs(c, seed=None):
    """operands of one case (CPU): feats [N,D] bf16, S [P,D] fp32, per block ("" node, "s" super) W bits / b (plain) and
    Wc bits / bc (centred), gamma / beta (None: instance).  shift: a bias of mean `shift` (|row mean| / std >= 100: the
    products have a standard deviation ~ 1); zero_row: the last row of feats and of S zero, and both biases zero."""
    lay = layout(c.layout)
    tg = torch.Generator().manual_seed(seed if seed is not None else 131 * lay.N + 7 * c.D + c.F)
    A = (torch.relu(torch.randn(lay.N, c.D, generator=tg)) + 0.3 * torch.rand(1, c.D, generator=tg)).to(torch.bfloat16)
    S = torch.randn(lay.P, c.D, generator=tg)
    if c.zero_row:
        A[-1] = 0
        S[-1] = 0
    inp = dict(lay=lay, feats=A, S=S, eps=EPS_NORM)
    for k in ("", "s"):
        W32 = torch.randn(c.F, c.D, generator=tg) / c.D ** 0.5
        b = torch.randn(c.F, generator=tg) * 0.1 + c.shift
        if c.zero_row:
            b = torch.zeros(c.F)
        g = be = None
        if c.norm == "layer":
            g = torch.rand(c.F, generator=tg) + 0.5
            g[3::8] *= -1.0
            be = torch.randn(c.F, generator=tg) * 0.5
        wc, bc = center(W32, b)
        inp.update({"W" + k: W32.to(torch.bfloat16), "b" + k: b, "Wc" + k: wc, "bc" + k: bc, "g" + k: g, "be" + k: be})
    return inp


def _row(v, like):
    return None if v is None else v.to(like.device).double()


def rownorm_ref(a64, w64, b, gamma, beta, eps, route, relu=True):
    """(want, delta) [M,F] float64.  a64 [M,K], w64 [F,K] hold the values the kernel multiplies; route: "fused" (w64 / b are the
    centred operands), "materialise" (the plain ones) or "rows" (no GEMM: a64 IS the fp32 matrix y, w64 / b None)"""
    if route == "rows":
        y, dd = a64, torch.zeros_like(a64)
    else:
        K = a64.shape[1]
        b64 = b.to(a64.device).double()
        y = a64 @ w64.t() + b64
        dd = dot_delta(a64.abs() @ w64.abs().t() + b64.abs(), K)
    F = y.shape[1]
    mean = y.mean(1, keepdim=True)
    d = y - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    g = _row(gamma, y) if gamma is not None else torch.ones(F, dtype=torch.float64, device=y.device)
    be = _row(beta, y) if beta is not None else torch.zeros(F, dtype=torch.float64, device=y.device)
    z = d * rstd * g + be
    if route == "fused":
        v = y.abs()
        e_d = dd + dd.mean(1, keepdim=True) + (F + 2.0) * EPS32 * (v + dd).mean(1, keepdim=True)
    else:
        v = (y - y[:, :1]).abs()
        e_d = dd + dd.mean(1, keepdim=True) + EPS32 * (3.0 * v + (F + 2.0) * v.mean(1, keepdim=True))
    dv = 2.0 * torch.sqrt(var) * torch.sqrt((e_d * e_d).mean(1, keepdim=True)) + (e_d * e_d).mean(1, keepdim=True)
    x = (dv + 3.0 * (F + 2.0) * EPS32 * ((v + dd) ** 2).mean(1, keepdim=True)) / (var + eps)
    rel = torch.where(x < 1.0, 1.0 / torch.sqrt((1.0 - x).clamp_min(1e-300)) - 1.0, torch.full_like(x, float("inf"))) + 10.0 * EPS32
    delta = g.abs() * rstd * (e_d * (1.0 + rel) + d.abs() * rel) + 4.0 * EPS32 * ((d * rstd * g).abs() + be.abs())
    return (torch.relu(z) if relu else z), delta


def residual_mean_bound(a64, wc64, bc):
    """m_w [M]: what the rounding of the centred operands can leave of a row's mean (module docstring)"""
    return H16 / (1.0 - H16) * (a64.abs() @ wc64.abs().mean(0)) + EPS32 * bc.double().abs().mean()


def pool(val, seg, P):
    out = torch.zeros(P, val.shape[1], dtype=val.dtype, device=val.device)
    return out.index_reduce_(0, seg, val, "amax", include_self=True)


def pair_ref(inp, route, dev="cpu"):
    """(pooled want [P,F], its tolerance, super want [P,F], its delta) of one route, float64 on `dev`"""
    k = "c" if route == "fused" else ""
    seg = torch.from_numpy(np.ascontiguousarray(inp["lay"].bbox_idx)).to(dev)
    P = inp["lay"].P
    val, delta = rownorm_ref(widen(inp["feats"].to(dev)), widen(inp["W" + k].to(dev)), inp["b" + k], inp["g"], inp["be"], inp["eps"], route)
    sval, sdelta = rownorm_ref(bf(inp["S"].to(dev)), widen(inp["W" + k + "s"].to(dev)), inp["b" + k + "s"], inp["gs"], inp["bes"],
                               inp["eps"], route)
    return pool(val, seg, P), pool(delta, seg, P), sval, sdelta


# ---------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' arithmetic order (CPU)
# ---------------------------------------------------------------------------------------------
def _butterfly(q, width):
    """q [M, width] fp32 -> the sum every lane holds after xor-shuffles of width / 2, ..., 1 (column 0 taken)"""
    idx = torch.arange(width)
    o = width // 2
    while o > 0:
        q = q + q[:, idx ^ o]
        o //= 2
    return q[:, :1]


def _acc32(a_bf, w_bits, b):
    return a_bf.float() @ w_bits.float().t() + b.float()


def emulate_fused(a_bf, wc_bits, bc, gamma, beta, eps, relu=True):
    """k_hfusion_rows8_rn: sums of d and d^2 per lane over the column tiles, butterflies over 32, var = mean(d^2) - m^2"""
    d = _acc32(a_bf, wc_bits, bc)
    F = d.shape[1]
    q, s = torch.zeros(d.shape[0], 32), torch.zeros(d.shape[0], 32)
    for ct in range(F // 64):
        a0, a1 = d[:, 64 * ct:64 * ct + 32], d[:, 64 * ct + 32:64 * ct + 64]
        q = a0 * a0 + (a1 * a1 + q)
        s = s + (a0 + a1)
    inv_f = torch.tensor(1.0 / F)
    m = _butterfly(s, 32) * inv_f
    rstd = 1.0 / torch.sqrt((_butterfly(q, 32) * inv_f - m * m).clamp_min(0.0) + torch.tensor(eps))
    z = d * rstd + (-m * rstd)
    if gamma is not None:
        z = z * gamma.float() + beta.float()
    return torch.relu(z) if relu else z


def emulate_rows(y32, gamma, beta, eps, relu=True):
    """yolat_rownorm_act / k_rownorm_act_h on an fp32 matrix: centred on the first element, column c in lane c mod 64"""
    M, C = y32.shape
    v = y32 - y32[:, :1]
    pad = (-C) % 64
    lanes = torch.cat([v, torch.zeros(M, pad)], 1).view(M, -1, 64)
    s = torch.zeros(M, 64)
    for i in range(lanes.shape[1]):
        s = s + lanes[:, i]
    ms = _butterfly(s, 64) * torch.tensor(1.0 / C)
    d = v - ms
    dl = torch.cat([d, torch.zeros(M, pad)], 1).view(M, -1, 64)
    q = torch.zeros(M, 64)
    for i in range(dl.shape[1]):
        q = dl[:, i] * dl[:, i] + q
    rstd = 1.0 / torch.sqrt(_butterfly(q, 64) * torch.tensor(1.0 / C) + torch.tensor(eps))
    z = d * rstd
    if gamma is not None:
        z = z * gamma.float() + beta.float()
    return torch.relu(z) if relu else z


def emulate_materialise(a_bf, w_bits, b, gamma, beta, eps):
    """the materialising route: the tile GEMM with the bias into fp32, then yolat_rownorm_act"""
    return emulate_rows(_acc32(a_bf, w_bits, b), gamma, beta, eps)


def emulate_pair(inp, route):
    """(pooled [P,F], super [P,F]) fp32 of one route"""
    seg = torch.from_numpy(np.ascontiguousarray(inp["lay"].bbox_idx))
    P = inp["lay"].P
    S = inp["S"].to(torch.bfloat16)
    if route == "fused":
        val = emulate_fused(inp["feats"], inp["Wc"], inp["bc"], inp["g"], inp["be"], inp["eps"])
        return pool(val, seg, P), emulate_fused(S, inp["Wcs"], inp["bcs"], inp["gs"], inp["bes"], inp["eps"])
    val = emulate_materialise(inp["feats"], inp["W"], inp["b"], inp["g"], inp["be"], inp["eps"])
    return pool(val, seg, P), emulate_materialise(S, inp["Ws"], inp["bs"], inp["gs"], inp["bes"], inp["eps"])


# ---------------------------------------------------------------------------------------------
# planted defects: each returns the node half's [N,F] activations of a wrong kernel, fp32
# ---------------------------------------------------------------------------------------------
def _finish(d, rstd, gamma, beta):
    z = d * rstd
    if gamma is not None:
        z = z * gamma.float() + beta.float()
    return torch.relu(z)


def defect_var_e2(inp):
    """un-centred weights, a mean sweep, and the variance as E[y^2] - mean^2 (fp32 cancellation at |mean| >> std)"""
    y = _acc32(inp["feats"], inp["W"], inp["b"])
    mean = y.mean(1, keepdim=True)
    var = ((y * y).mean(1, keepdim=True) - mean * mean).clamp_min(0.0)
    return _finish(y - mean, 1.0 / torch.sqrt(var + torch.tensor(inp["eps"])), inp["g"], inp["be"])


def defect_uncentred(inp):
    """the fused kernel handed the PLAIN weights: no mean sweep, the accumulator taken for the deviation"""
    y = _acc32(inp["feats"], inp["W"], inp["b"])
    var = (y * y).mean(1, keepdim=True)
    return _finish(y, 1.0 / torch.sqrt(var + torch.tensor(inp["eps"])), inp["g"], inp["be"])


def defect_unbiased(inp):
    """the variance divided by F - 1"""
    d = _acc32(inp["feats"], inp["Wc"], inp["bc"])
    var = (d * d).sum(1, keepdim=True) / (d.shape[1] - 1)
    return _finish(d, 1.0 / torch.sqrt(var + torch.tensor(inp["eps"])), inp["g"], inp["be"])


def defect_no_mean_sweep(inp):
    """the fused kernel on the centred bf16 weights WITHOUT the sum of d: the residual row mean of the rounding stays in"""
    d = _acc32(inp["feats"], inp["Wc"], inp["bc"])
    var = (d * d).mean(1, keepdim=True)
    return _finish(d, 1.0 / torch.sqrt(var + torch.tensor(inp["eps"])), inp["g"], inp["be"])


DEFECTS = {"var_e2": (defect_var_e2, "materialise"), "uncentred": (defect_uncentred, "materialise"),
           "unbiased": (defect_unbiased, "fused"), "no_mean_sweep": (defect_no_mean_sweep, "fused")}      # name -> (wrong kernel, the route whose reference it is held to)


# ---------------------------------------------------------------------------------------------
# the classifier's row norm: fp32 rows in, bf16 out
# ---------------------------------------------------------------------------------------------
ROWS_CASES = tuple((C, M, norm) for C in (256, 512) for M in (1, 63, 65) for norm in ("layer", "instance"))


def rows_inputs(C, M, norm):
    tg = torch.Generator().manual_seed(977 * C + M)
    Y = torch.randn(M, C, generator=tg) * 3.0 + torch.randn(M, 1, generator=tg) * 20.0
    g = be = None
    if norm == "layer":
        g = torch.rand(C, generator=tg) + 0.5
        g[3::8] *= -1.0
        be = torch.randn(C, generator=tg) * 0.5
    return dict(Y=Y, g=g, be=be, eps=EPS_NORM)


def rows_ref(inp, dev="cpu"):
    """(want [M,C] float64, tolerance) of k_rownorm_act_h: the float64 norm, and the envelope of ONE bf16 rounding of a value
    within delta of it (half a bf16 spacing + delta: a second rounding or a truncating store does not fit)"""
    z, delta = rownorm_ref(inp["Y"].to(dev).double(), None, None, inp["g"], inp["be"], inp["eps"], "rows")
    return z, store_envelope(z, delta)


def emulate_rows_h(inp, store="nearest"):
    z = emulate_rows(inp["Y"], inp["g"], inp["be"], inp["eps"])
    return truncate_bf16(z) if store == "truncate" else z.to(torch.bfloat16)


def worst(name, got, want, tol):
    """prints and returns the worst error / tolerance and the number of elements outside (NaN counts as outside)"""
    err = (got.double() - want).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print("ratio %-52s %.3f" % (name, ratio))
    return ratio, int(bad.sum())
