"""float64 references, per-element envelopes and fp32 emulations for the fp32 graph ops of the training step:
csr_mean_fwd / _bwd, edge_scatter_bwd, yolat_edge_uv_sums / _v, yolat_edge_uv_lin1_fwd (csrc/edge_ops.hip), BnCsrGrad
(csrc/bn_csr.hip) and the segment ops (csrc/segment.hip).  CPU only: torch and numpy, no import of the extension.
tests/test_graph_ref_host.py checks every claim made here; tests/test_gpu_fp32_graph_ops.py holds the kernels to these
envelopes.

Every tolerance is per element and formed from u = 2^-24 and the magnitudes that element's arithmetic goes through,
following the kernel source; nothing is scaled by a tensor maximum.  Inputs are full-mantissa fp32 values (not on the
bfloat16 grid of bf16_ref): a (scale, shift) prologue is then ONE rounded fma, which costs u |t| per term.  A ReLU in a
FORWARD is continuous, |relu(a) - relu(b)| <= |a - b|, and needs no mask.  A ReLU mask in a BACKWARD is `fmaf(y, sc, sh) >
0` in the kernels: one correct rounding keeps the sign of the exact value, and so does the float64 `y sc + sh` (an exact
product, one rounded sum), so on fp32 operands the two masks are the SAME (relu_mask_is_exact; the host test shows it for
every case used).  The next BatchNorm's sums therefore carry no kink term.  The statistics and dY of the BatchNorm behind
the aggregation keep the kink terms of the bf16 test's rule (the full magnitude of the terms with |t| <= KINK, at most
KINK_SHARE of the elements, checked per case), although the same argument holds for that mask: they widen those bounds.

The references are torch code that runs where its operands live (the GPU tests evaluate them in float64 on the device);
the emulations are numpy / torch fp32 on the CPU, written from the kernel source, and take a `defect` argument: the host
tests show that every envelope accepts the emulation and rejects every planted defect.
"""
import numpy as np
import torch

# (KINK_SHARE, group_stats_ref, in_degree and kink_share are handed on to the two test files)
from bf16_ref import (EPS32, KINK_SHARE, bn_relu_bwd_ref, chain, csr_mean_bwd_ref, dot_delta, group_stats_ref, hub, in_degree,
                      kink_share, uniform)

U = EPS32
SLACK = 1.0 + 2.0 ** -20    # second-order terms of a first-order bound


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# graphs and segment sizes
# ---------------------------------------------------------------------------------------------
def ladder(n_max=40, N=45, seed=0):
    """(src, dst) int64: node n has in-degree exactly n for n = 0 .. n_max, `src` is a seeded permutation of the same
    multiset (so node n has out-degree n too), nodes above n_max have no edge, the edge order is shuffled.
    E = n_max (n_max + 1) / 2 = 820 at the defaults; N = 45 is no multiple of 4 or 16, so the last workgroup of every
    node-mapped kernel is partial.  A run of n = 8 k + t rows is k full eight-row trips and a t-row tail: every tail
    length 0..7 occurs behind 0..4 trips, and n = 40 is five trips without a tail."""
    if N <= n_max:
        raise ValueError("ladder(%d, %d): needs N > n_max" % (n_max, N))
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(n_max + 1, dtype=np.int64), np.arange(n_max + 1))
    src = rng.permutation(dst)
    order = rng.permutation(len(dst))
    return src[order].astype(np.int64), dst[order].astype(np.int64)


def segment_ladder(seed=0, n_max=40, big=300):
    """int64 [n_max + 2]: the segment sizes 0, 1, .., n_max in a seeded order and one segment of `big` rows among them;
    the first and the last segment are non-empty (what build_graph expects of a bbox_idx)."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.arange(n_max + 1), [big]]).astype(np.int64)
    sizes = sizes[rng.permutation(len(sizes))]
    for end in (0, -1):
        if sizes[end] == 0:
            j = len(sizes) // 2 if sizes[len(sizes) // 2] != 0 else len(sizes) // 2 + 1
            sizes[end], sizes[j] = sizes[j], sizes[end]
    return sizes


def segment_ids(sizes):
    """(bbox_idx int64 [N], seg_ptr int64 [P + 1]) of the segment sizes"""
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes), np.concatenate([[0], np.cumsum(sizes)])


def csr_of(src, dst, N):
    """(order, row_ptr, col_ptr, slots) int64: the stable sort by destination, the CSR row pointers, and the CSC by source
    over the CSR slots (ascending slots per source) — the structure build_graph / ensure_csc derive on the device"""
    order = np.argsort(dst, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int64)
    s_csr = src[order]
    slots = np.argsort(s_csr, kind="stable").astype(np.int64)
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int64)
    return order, row_ptr, col_ptr, slots


# ---------------------------------------------------------------------------------------------
# inputs: full-mantissa fp32
# ---------------------------------------------------------------------------------------------
def randn32(shape, seed, scale=1.0, shift=0.0):
    """fp32 normal draws: 24 significant bits, so NOT bfloat16 values (has_full_mantissa)"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def has_full_mantissa(t, share=0.9):
    """more than `share` of the elements of the fp32 tensor have a set bit among the low 16 of their mantissa, i.e. are
    no bfloat16 values"""
    bits = t.detach().cpu().contiguous().view(torch.int32) & 0xFFFF
    return float((bits != 0).double().mean()) > share


def pro_scale_shift(C, seed):
    """(scale, shift) fp32 [C] of a BatchNorm prologue, full mantissa: scale in [0.5, 1.5), shift ~ 0.3 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3


def bn_bwd_inputs32(M, C, seed):
    """bf16_ref.bn_bwd_inputs with FULL-MANTISSA fp32 Y (and no dZ: the gradient here is gathered from d_out): Y [M,C]
    fp32 ~ 1.5 N(0,1) + 0.3; save_mean, save_invstd, scale = gamma invstd, shift = beta - mean scale fp32 [C] from the
    REAL batch statistics of Y; |beta| >= 1/16 keeps a single-row batch off the ReLU kink.
    Condition (host test, every case used): kink_share(Y, scale, shift) <= KINK_SHARE."""
    g = torch.Generator().manual_seed(seed)
    Y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).float()
    y = Y.double()
    mean = y.mean(0)
    invstd = 1.0 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, generator=g).double() + 0.5
    beta = (torch.rand(C, generator=g).double() * 0.5 + 0.0625) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return Y, mean.float(), invstd.float(), (gamma * invstd).float(), (beta - mean * gamma * invstd).float()


# ---------------------------------------------------------------------------------------------
# envelopes of the run sums
# ---------------------------------------------------------------------------------------------
def run_sum_tol(mag, deg):
    """A sum of `deg` fp32 terms added one by one (k_edge_uv_sums, k_edge_scatter_bwd: s += v in slot order, deg
    roundings, the first of them exact): (deg + 2) u sum |terms|.  mag: that magnitude sum, deg broadcastable to it."""
    return (deg + 2.0) * U * mag


def mean_tol(mag, deg, divides=False):
    """The mean of `deg` fp32 terms.  edge_ops.hip (k_csr_mean_fwd, _v4): the sum, then yl_mul_rn(s, inv) with inv =
    fl(1 / max(deg, 1)) — the sum's deg roundings, the reciprocal's and the product's: (deg + 3) u sum |terms| / deg.
    segment.hip (k_segment_mean_fwd) divides, s / (float)cnt, one rounding less: (deg + 2) u sum |terms| / deg."""
    return (deg + (2.0 if divides else 3.0)) * U * mag / deg.clamp_min(1)


def accumulate_tol(base, total):
    """the accumulating store `s += *o; *o = s` rounds once: u (|base| + |sum|)"""
    return U * (base.double().abs() + total.abs())


def prologue64(h, scale, shift, relu):
    """(value, magnitude of the value, magnitude of the pre-ReLU t = h scale + shift) in float64; no prologue: h itself
    and a zero third member (no fma, no rounding)"""
    h = h.double()
    if scale is None:
        return h, h.abs(), torch.zeros_like(h)
    t = h * scale.double() + shift.double()
    v = torch.relu(t) if relu else t
    return v, v.abs(), t.abs()


def _node_sum(v, idx, N):
    return torch.zeros(N, v.shape[1], dtype=torch.float64, device=v.device).index_add_(0, idx, v)


def csr_mean_fwd_ref(h, scale, shift, relu, dst, N, base=None, divides=False):
    """out (+)= mean over the run of pro(h), float64, rows h [E,C] with their run ids dst [E] (any order of runs; the
    result does not depend on it).  Tolerance per run and column, from k_csr_mean_fwd_v4 as written:
        s += fmaxf(fmaf(v, sc, sh), floor)   the fma rounds once (u |t| per term; the ReLU is continuous), the additions
                                             deg times
        s = yl_mul_rn(s, inv)                reciprocal and product
        s += *o                              accumulating: once more
      = mean_tol(sum |pro(h)|, deg) + u sum |t| / deg  (+ accumulate_tol).
    Returns (want, tol, deg float64 [N])."""
    v, mag_v, mag_t = prologue64(h, scale, shift, relu)
    deg = torch.bincount(dst, minlength=N).double()
    d1 = deg.clamp_min(1)[:, None]
    mean = _node_sum(v, dst, N) / d1
    tol = mean_tol(_node_sum(mag_v, dst, N), deg[:, None], divides) + U * _node_sum(mag_t, dst, N) / d1
    tol = tol * SLACK
    if base is None:
        return mean, tol, deg
    return mean + base.double(), tol + accumulate_tol(base, mean), deg


def csr_mean_bwd_fp32(d_out, dst, N):
    """k_csr_mean_bwd / _v4 as written, in torch fp32: dM[q] = d_out[dst_q] * fl(1 / max(deg, 1)) — an IEEE division and
    one rounded product, no fma to contract: the kernel must return these BITS.  (The float64 quotient d_out / deg lies
    within 2 u |quotient| of it: csr_mean_bwd_ref.)"""
    deg = torch.bincount(dst, minlength=N).clamp_min(1)
    inv = (torch.ones(N, dtype=torch.float32) / deg.cpu().float()).to(d_out.device)      # IEEE division, on the CPU
    return d_out.float()[dst] * inv[dst][:, None]


def edge_scatter_bwd_ref(dG, Cin, src, dst, N, base=None):
    """dX[n] (+)= sum_{dst_q = n} dG[q, :Cin] + sum_{src_q = n} dG[q, Cin:2 Cin] in float64.  k_edge_scatter_bwd(_v4) adds
    both runs into ONE accumulator, deg_in + deg_out additions: (deg_in + deg_out + 2) u sum |terms| (+ accumulate_tol).
    Returns (want, tol)."""
    a, b = dG[:, :Cin].double(), dG[:, Cin:2 * Cin].double()
    want = _node_sum(a, dst, N) + _node_sum(b, src, N)
    mag = _node_sum(a.abs(), dst, N) + _node_sum(b.abs(), src, N)
    deg = (torch.bincount(dst, minlength=N) + torch.bincount(src, minlength=N)).double()[:, None]
    tol = run_sum_tol(mag, deg)
    if base is None:
        return want, tol
    return want + base.double(), tol + accumulate_tol(base, want)


def edge_uv_sums_ref(dH, src, dst, N):
    """(dU, tol_dU, dV, tol_dV): dU[n] = sum over the in-edges' rows of dH, dV[n] = over the out-edges' rows, float64;
    each a run sum of its own in k_edge_uv_sums: run_sum_tol"""
    h = dH.double()
    din = torch.bincount(dst, minlength=N).double()[:, None]
    dout = torch.bincount(src, minlength=N).double()[:, None]
    return (_node_sum(h, dst, N), run_sum_tol(_node_sum(h.abs(), dst, N), din),
            _node_sum(h, src, N), run_sum_tol(_node_sum(h.abs(), src, N), dout))


def edge_uv_lin1_ref(UV, src, dst, attr, wc4, b1):
    """H1[q] = U[dst_q] + V[src_q] + Wc4 . attr_q + b1 on a GIVEN UV [N,128] = (U | V), float64.  k_edge_uv_lin1 rounds
    six times (u + v, four fmas, + b1), each relative to a partial sum no larger than S = |u| + |v| + |attr| . |Wc4| +
    |b1|: delta = 6 u S.  Returns (want, delta) — delta is also the values' bound for group_stats_ref."""
    C = wc4.shape[0]
    Uu, Vv = UV[:, :C].double(), UV[:, C:2 * C].double()
    bb = b1.double() if b1 is not None else torch.zeros(C, dtype=torch.float64, device=UV.device)
    a, w = attr.double(), wc4.double()
    want = Uu[dst] + Vv[src] + a @ w.t() + bb
    S = Uu[dst].abs() + Vv[src].abs() + a.abs() @ w.abs().t() + bb.abs()
    return want, 6.0 * U * S * SLACK


def segment_mean_bwd_tol(want):
    """k_segment_mean_bwd: dY[p] / (float)cnt, one IEEE division of two fp32 values: u |want|"""
    return U * want.abs()


# ---------------------------------------------------------------------------------------------
# BatchNorm + ReLU + mean aggregation backward (bn_csr.hip)
# ---------------------------------------------------------------------------------------------
BCS_ROWS = 640              # rows per workgroup of k_bn_csr_partial
BCL_WGS = 512               # workgroups of k_bn_csr_l2_bwd at most


def l2_tiles(E):
    """(tiles, tiles per workgroup, workgroups) of yolat_bn_csr_l2_bwd, restated from its host code"""
    tiles = _cdiv(E, 64)
    per = _cdiv(tiles, min(tiles, BCL_WGS))
    return tiles, per, _cdiv(tiles, per)


def bn_csr_stats_ref(d_out, dst, N, Y, mean, invstd, scale, shift):
    """The statistics of BnCsrGrad.stats() in float64 and their tolerances.  g = [z > 0] d_out[dst] / deg; dbeta = sum g,
    dgamma = sum g xhat, (c1, c2) = sums / E.  k_bn_csr_partial: fp32 over a block of 640 rows (any order inside it), a
    term carries fl(1 / deg), the product, and for g xhat three more roundings; k_bn_csr_finalize: float64 across the
    blocks, one rounding to fp32:
        (min(E, 640) + 8) u sum |terms|  + the full magnitude of the terms within KINK of the ReLU kink
    (the rule of test_gpu_bf16_storage_ops.py::test_bn_csr_grad_bf16_storage_matches_fp64, no bfloat16 terms).
    Returns (ref dict of bn_relu_bwd_ref, g0 = d_out[dst] / deg, tol_dbeta, tol_dgamma)."""
    E = Y.shape[0]
    g0 = csr_mean_bwd_ref(d_out, dst, N)
    ref = bn_relu_bwd_ref(g0, Y, mean, invstd, scale, shift, True)
    unsure = (~ref["sure"]).double()
    n_blk = min(E, BCS_ROWS)
    tol_b = (n_blk + 8) * U * ref["g"].abs().sum(0) + (g0.abs() * unsure).sum(0)
    tol_g = (n_blk + 8) * U * (ref["g"] * ref["xhat"]).abs().sum(0) + ((g0 * ref["xhat"]).abs() * unsure).sum(0)
    return ref, g0, tol_b, tol_g


def bn_csr_dy_ref(g0, Y, mean, invstd, scale, shift, coef):
    """dY = scale (g - c1 - xhat c2) in float64 from the kernel's OWN fp32 (c1 | c2) = coef, and its bound for the fp32
    BnCsrOpT::one: ten roundings (fl(1 / deg), g w, y - mu, . is, . k2, g - k1, - ., sc ., and two spare for the second
    order), each relative to an intermediate no larger than |scale| (|g| + |c1| + |xhat c2|); + |scale g0| on the kink.
    Returns (dY, d_dY)."""
    ref = bn_relu_bwd_ref(g0, Y, mean, invstd, scale, shift, True, coef=coef)
    sc = scale.double().abs()
    unsure = (~ref["sure"]).double()
    d_dY = 10.0 * U * sc * (ref["g"].abs() + ref["c1"].abs() + (ref["xhat"] * ref["c2"]).abs()) + sc * g0.abs() * unsure
    return ref["dY"], d_dY


def bn_csr_consumers_ref(dY, d_dY, A, a_scale, a_shift, a_relu, W):
    """The consumers of dY [E,C], float64, with A1 = pro(A) [E,K] (one fma: |dA1| <= u |t|, ReLU continuous) and the
    Linear's weight W [C,K]:
        dW = dY^T . A1      d_dY^T . |A1| + |dY|^T . u |t| + 2 (E + 2) u |dY|^T . |A1|
        db = sum dY         sum d_dY + (E + 2) u sum |dY|
        dA = dY . W         d_dY . |W| + dot_delta(|dY| . |W|, C)
    (E + 2) u bounds E additions in ANY order — tiles in registers, workgroups' slabs, split rows; the factor 2 on the
    two matrix-core products is dot_delta's allowance for their undocumented internal order.
    Returns dict(dW, tol_dW, db, tol_db, dA, tol_dA, A1, t_abs)."""
    E, C = dY.shape
    A1, mag1, mag_t = prologue64(A, a_scale, a_shift, a_relu)
    w = W.double()
    ady = dY.abs()
    return dict(dW=dY.t() @ A1, tol_dW=(d_dY.t() @ mag1 + U * (ady.t() @ mag_t) + 2.0 * (E + 2) * U * (ady.t() @ mag1)) * SLACK,
                db=dY.sum(0), tol_db=(d_dY.sum(0) + (E + 2) * U * ady.sum(0)) * SLACK,
                dA=dY @ w, tol_dA=(d_dY @ w.abs() + dot_delta(ady @ w.abs(), C)) * SLACK)


def next_bn_ref(dA_stored, A, a_scale, a_shift, m1, is1):
    """The next BatchNorm's backward statistics out of k_bn_csr_l2_bwd, judged from the kernel's STORED dA (its
    contract): gp = [A a_scale + a_shift > 0] dA, sums of gp and gp xh1 with xh1 = (A - m1) is1, float64.  fp32 over one
    workgroup's 64 ceil(tiles / 512) rows, float64 across:  (64 ceil(tiles / 512) + 6) u sum |terms|, and nothing else:
    the kernel's mask fmaf(A, a_scale, a_shift) > 0 is the float64 one (relu_mask_is_exact), there is no kink term.
    Returns (dbeta, tol, dgamma, tol)."""
    E = A.shape[0]
    z = A.double() * a_scale.double() + a_shift.double()
    d = dA_stored.double()
    gp = d * (z > 0)
    xh = (A.double() - m1.double()) * is1.double()
    _, per, _ = l2_tiles(E)
    rows = 64 * per
    t1 = (rows + 6) * U * gp.abs().sum(0)
    t2 = (rows + 6) * U * (gp * xh).abs().sum(0)
    return gp.sum(0), t1, (gp * xh).sum(0), t2


def bn_csr_inputs(N, E, seed):
    """The operands of one BnCsrGrad case, all full-mantissa fp32 on the CPU: dict(Y, mean, invstd, scale, shift (the
    BatchNorm behind the aggregation, real statistics), d_out [N,64], A [E,64], a_scale, a_shift (the prologue in front
    of A), W [64,64], m1, is1 (the next BatchNorm's saved statistics)).
    Conditions (host test): kink_share(Y, scale, shift) <= KINK_SHARE; relu_mask_is_exact for both prologues."""
    Y, mean, invstd, scale, shift = bn_bwd_inputs32(E, 64, seed)
    a_scale, a_shift = pro_scale_shift(64, seed + 3)
    return dict(Y=Y, mean=mean, invstd=invstd, scale=scale, shift=shift, d_out=randn32((N, 64), seed + 2),
                A=randn32((E, 64), seed + 1), a_scale=a_scale, a_shift=a_shift, W=randn32((64, 64), seed + 4, 1 / 8),
                m1=randn32((64,), seed + 5, 0.2),
                is1=torch.rand(64, generator=torch.Generator().manual_seed(seed + 6)) + 0.5)


def emulate_bn_csr(inp, dst, N, with_next=True, defect=None):
    """bn_csr.hip in torch fp32 on the CPU, statement by statement for the element-wise part (torch's CPU kernels round
    every operation, nothing is contracted) and with the kernels' partition of the sums: k_bn_csr_partial's blocks of
    640 rows in fp32 and float64 across them; k_bn_csr_l2_bwd's workgroups of `per` 64-row tiles, every tile's product
    added to the workgroup's fp32 accumulators, the workgroups' slabs added in fp32 (float64 across for the next
    BatchNorm).  dst: int64 CSR-ordered [E].
    defect: None; "tile_loss": dW, db and the next BatchNorm's sums of a workgroup keep only its LAST tile (the
    accumulators are not carried from tile to tile) — invisible while every workgroup owns one tile (E <= 32768);
    "row_dup": the last row of dY is a copy of the row before (a clamped re-read that is not masked);
    "no_inv_deg": the gathered gradient is not divided by the degree.
    Returns dict(dbeta, dgamma, coef, dW, db, dA, next_dbeta, next_dgamma, next_coef) fp32."""
    f = torch.float32
    Y, A = inp["Y"].float(), inp["A"].float()
    E = Y.shape[0]
    mu, istd, sc, sh = [inp[k].float() for k in ("mean", "invstd", "scale", "shift")]
    deg = torch.bincount(dst, minlength=N).clamp_min(1)
    inv = torch.ones(N, dtype=f) / deg.float()
    g = inp["d_out"].float()[dst]
    if defect != "no_inv_deg":
        g = g * inv[dst][:, None]
    z = (Y.double() * sc.double() + sh.double()).float()                  # fmaf: one rounding
    g = torch.where(z > 0, g, torch.zeros_like(g))
    xh = (Y - mu) * istd

    def blocks(t, rows):                                                 # fp32 inside a block, float64 across
        acc = torch.zeros(t.shape[1], dtype=torch.float64)
        for r0 in range(0, E, rows):
            acc += t[r0:r0 + rows].sum(0, dtype=f).double()
        return acc
    s1, s2 = blocks(g, BCS_ROWS), blocks(g * xh, BCS_ROWS)
    coef = torch.cat([(s1 / E).float(), (s2 / E).float()])
    k1, k2 = coef[:64], coef[64:]
    dY = sc * (g - k1 - xh * k2)
    if defect == "row_dup" and E >= 2:
        dY = dY.clone()
        dY[-1] = dY[-2]
    A1 = torch.relu((A.double() * inp["a_scale"].double() + inp["a_shift"].double()).float())
    W = inp["W"].float()
    dA = dY @ W
    _, per, wgs = l2_tiles(E)
    dW = torch.zeros(64, 64, dtype=f)
    db = torch.zeros(64, dtype=f)
    n1, n2 = torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    za = (A.double() * inp["a_scale"].double() + inp["a_shift"].double()).float()
    gp = torch.where(za > 0, dA, torch.zeros_like(dA))
    xh1 = (A - inp["m1"].float()) * inp["is1"].float()
    for w in range(wgs):
        pw, pb = torch.zeros(64, 64, dtype=f), torch.zeros(64, dtype=f)
        p1, p2 = torch.zeros(64, dtype=f), torch.zeros(64, dtype=f)
        for t in range(w * per, min((w + 1) * per, _cdiv(E, 64))):
            r = slice(64 * t, min(64 * t + 64, E))
            if defect == "tile_loss":
                pw, pb, p1, p2 = torch.zeros_like(pw), torch.zeros_like(pb), torch.zeros_like(p1), torch.zeros_like(p2)
            pw = pw + dY[r].t() @ A1[r]
            pb = pb + dY[r].sum(0, dtype=f)
            p1 = p1 + gp[r].sum(0, dtype=f)
            p2 = p2 + (gp[r] * xh1[r]).sum(0, dtype=f)
        dW, db = dW + pw, db + pb
        n1, n2 = n1 + p1.double(), n2 + p2.double()
    out = dict(dbeta=s1.float(), dgamma=s2.float(), coef=coef, dW=dW, db=db, dA=dA)
    if with_next:
        out.update(next_dbeta=n1.float(), next_dgamma=n2.float(), next_coef=torch.cat([(n1 / E).float(), (n2 / E).float()]))
    return out


# ---------------------------------------------------------------------------------------------
# fp32 emulations of the run sums (numpy)
# ---------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 numpy arrays, correctly rounded: the product of two fp32 values is exact in float64, its sum
    with c is rounded to float64 with the residual known (TwoSum), and the final rounding to fp32 is corrected where the
    float64 sum sits exactly on an fp32 tie while the residual is not zero (the only place double rounding can bite: a tie
    is itself a float64 value, so none lies strictly between the float64 sum and the true one)."""
    a, b, c = [np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c)]
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                     # s + e == p + c exactly
        lo = s.astype(np.float32)
        d = s - lo.astype(np.float64)                     # exact: two nearby float64 values
        nb = np.nextafter(lo, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & (np.abs(d) == np.abs(nb.astype(np.float64) - s))
        # at a tie the cast gave the even neighbour `lo`; the true value lies beyond the tie, on nb's side, iff the
        # residual points the way the float64 sum lies from lo
        away = tie & (e != 0) & (np.sign(e) == np.sign(d))
        out = np.where(away, nb, lo)
    return out.astype(np.float32)


def relu_mask_is_exact(a, scale, shift):
    """the fp32 mask fmaf(a, scale, shift) > 0 (correctly rounded: fma32) equals the float64 mask a scale + shift > 0 on
    every element of the fp32 operands: neither rounding moves a value across zero"""
    z32 = fma32(a.numpy(), scale.numpy()[None, :], shift.numpy()[None, :])
    z64 = a.double() * scale.double() + shift.double()
    return bool(np.array_equal(z32 > 0, (z64 > 0).numpy()))


def emulate_group_stats(h, rows=32):
    """(sum, M2 about the group mean) [G, C] fp32 per `rows`-row group of the fp32 values h [M, C] as k_edge_uv_lin1's
    statistics epilogue forms them, numpy fp32: sum in row order, mu = sum / cnt, then sum of fl(fl(v - mu)^2) in row
    order (the last group short)"""
    f = np.float32
    h = np.asarray(h, dtype=f)
    M, C = h.shape
    G = _cdiv(M, rows)
    s, m2 = np.zeros((G, C), dtype=f), np.zeros((G, C), dtype=f)
    for gi in range(G):
        blk = h[gi * rows:min(M, (gi + 1) * rows)]
        a = np.zeros(C, dtype=f)
        for r in blk:
            a = a + r
        mu = a / f(len(blk))
        b = np.zeros(C, dtype=f)
        for r in blk:
            d = r - mu
            b = b + d * d
        s[gi], m2[gi] = a, b
    return s, m2


RUN_DEFECTS = ("tail_reread", "drop_last", "tile_loss")


def emulate_run_sum(rows, ptr, trip=8, clamped=False, scale=None, shift=None, relu=False, init=None, defect=None,
                    tile=64):
    """fp32 sums [runs, C] over the runs [ptr[i], ptr[i + 1]) of the fp32 rows [E, C], added one row at a time in
    ascending order (what every run-sum kernel does whatever its unroll), numpy fp32.
    The unroll shape decides what a DEFECT does:
      trip = 8, clamped = False   k_csr_mean_fwd_v4, k_edge_uv_sums' dU loop, the segment kernels: full eight-row trips,
                                  then ONE tail of t = deg % 8 rows that loads 7 rows at clamped addresses (the segment
                                  kernels' tail is a rolled loop: it has no clamped loads to get wrong)
      trip = 4 or 8, clamped = True   k_edge_scatter_bwd_v4 (4), k_edge_uv_sums' dV loop (8): every trip loads `trip` rows at
                                  clamped addresses and adds the valid ones
    scale / shift / relu: the prologue fmaxf(fmaf(v, sc, sh), floor).  init [runs, C]: the accumulator's start (the second
    run of k_edge_scatter_bwd continues the first).
    defect: "tail_reread": the clamped loads of the last trip are all added (the `if (q + j < q1)` guard is missing): the
            run's last row enters 7 - t (clamped: trip - t) extra times;
            "drop_last": the last row of a run is not added;
            "tile_loss": the accumulator is cleared where a run crosses a multiple of `tile` rows (partial sums not
            carried from one tile of rows to the next).
    Without a defect the result does not depend on `trip` / `clamped`: the unroll shapes differ in what can go wrong, not in
    the order of the additions.  The run-sum kernels have no tiles of their own: "tile_loss" here stands for any loop
    that forgets what it has summed at a fixed row boundary; the mechanism itself (accumulators carried from tile to
    tile of one workgroup) is k_bn_csr_l2_bwd's and is modelled by emulate_bn_csr."""
    f = np.float32
    rows = np.asarray(rows, dtype=f)
    n = len(ptr) - 1
    out = np.zeros((n, rows.shape[1]), dtype=f) if init is None else np.array(init, dtype=f)
    if scale is not None:
        rows = fma32(rows, np.asarray(scale, dtype=f)[None, :], np.asarray(shift, dtype=f)[None, :])
        if relu:
            rows = np.maximum(rows, f(0))
    with np.errstate(all="ignore"):
        for i in range(n):
            q0, q1 = int(ptr[i]), int(ptr[i + 1])
            s = out[i].copy()
            last = q1 - 1 if defect == "drop_last" else q1
            for q in range(q0, last):
                if defect == "tile_loss" and q > q0 and q % tile == 0:
                    s = np.zeros_like(s)
                s = s + rows[q]
            if defect == "tail_reread" and q1 > q0:
                t = (q1 - q0) % trip
                extra = 0 if t == 0 else ((trip - t) if clamped else (trip - 1 - t))
                for _ in range(extra):
                    s = s + rows[q1 - 1]
            out[i] = s
    return out


def emulate_mean(sums, ptr, divides=False, defect=None):
    """the mean's last step on the fp32 run sums: yl_mul_rn(s, fl(1 / max(deg, 1))) (edge_ops.hip), or s / (float)max(cnt,
    1) (segment.hip: divides).  defect "deg_divisor": the divisor is deg, not max(deg, 1) — an empty run gives 0 x inf or
    0 / 0 = NaN where 0 is due."""
    f = np.float32
    deg = np.diff(np.asarray(ptr)).astype(f)
    if defect != "deg_divisor":
        deg = np.maximum(deg, f(1))
    with np.errstate(all="ignore"):
        if divides:
            return (np.asarray(sums, dtype=f) / deg[:, None]).astype(f)
        inv = (f(1) / deg).astype(f)
        return (np.asarray(sums, dtype=f) * inv[:, None]).astype(f)


def first_argmax(x, ptr, N):
    """(max, arg) per run and column with the FIRST (lowest) row winning ties, numpy; an empty run: value 0, arg N —
    k_segment_max_fwd's contract (torch_scatter semantics)"""
    x = np.asarray(x)
    P = len(ptr) - 1
    best = np.zeros((P, x.shape[1]), dtype=x.dtype)
    arg = np.full((P, x.shape[1]), N, dtype=np.int64)
    for p in range(P):
        r0, r1 = int(ptr[p]), int(ptr[p + 1])
        if r1 > r0:
            a = np.argmax(x[r0:r1], axis=0)               # numpy: the first occurrence
            best[p] = x[r0:r1][a, np.arange(x.shape[1])]
            arg[p] = r0 + a
    return best, arg


# ---------------------------------------------------------------------------------------------
# the cases of the GPU tests (the host tests run the emulations over the same ones)
# ---------------------------------------------------------------------------------------------
GRAPHS = {
    "tiny": lambda: (20,) + uniform(20, 7, seed=1),                      # E < 32
    "hub65": lambda: (300,) + hub(300, 2000, 65, seed=2),
    "hub150": lambda: (300,) + hub(300, 2000, 150, seed=3),
    "hub1000": lambda: (300,) + hub(300, 2000, 1000, seed=4),            # one 1000-row run, 130 empty nodes behind it
    "chain257": lambda: (257,) + chain(257),
    "ladder": lambda: (45,) + ladder(seed=6),
}

# row counts of the factorised first edge Linear: those of the bf16 twin
EDGE_CASES = [(1, "uniform"), (31, "uniform"), (33, "uniform"), (63, "uniform"), (64, "uniform"), (65, "uniform"),
              (1000, "uniform"), (4097, "uniform"), (1000, "hub150"), (4097, "hub1000")]

# (N, E, kind): the bf16 twin's cases and the two smallest E at which a workgroup of the one-kernel backward owns more
# than one tile: 513 tiles = two per workgroup, the last workgroup one; 1025 tiles = three per workgroup, the last two
BN_CSR_MULTI_TILE = [(4000, 32769, "uniform"), (4000, 65537, "hub1000")]
BN_CSR_CASES = [(50, 31, "uniform"), (64, 64, "uniform"), (64, 65, "uniform"), (64, 129, "uniform"), (300, 1000, "uniform"),
                (300, 1000, "hub150")] + BN_CSR_MULTI_TILE

SEGMENT_D = [128, 1152, 5]


def edge_case_graph(E, kind):
    """(N, src, dst) of an EDGE_CASES entry: a hub graph needs E >= 2 deg, below that the graph is uniform over 50 nodes"""
    if kind == "uniform":
        return (50,) + uniform(50, E, seed=E)
    return (300,) + hub(300, E, int(kind[3:]), seed=E)


def bn_csr_graph(N, E, kind):
    return uniform(N, E, seed=N + E) if kind == "uniform" else hub(N, E, int(kind[3:]), seed=N + E)
