"""float64 references, per-element envelopes and fp32 emulations for the ops that close a training step:
yolat_softmax_ce, yolat_adam_step, yolat_dropout_fwd / _bwd (csrc/loss_optim.hip) and the three GEMM forms of the
bf16_dense precision, yolat_bt_linear_fwd / _fwd_wt / _bwd_w (csrc/bf16_train.hip).  CPU only: torch and numpy, no
import of the extension.  tests/test_head_ref_host.py checks every claim made here; tests/test_gpu_head_ops.py and
tests/test_gpu_bt_gemm.py hold the kernels to these envelopes.

Every tolerance is per element and formed from u = 2^-24 (fp32 round to nearest) and the magnitudes that element's
arithmetic goes through, following the kernel source statement by statement; nothing is scaled by a tensor maximum.  The
emulations (numpy fp32, written from the kernel source) follow the kernels' order of operations and take a `defect`
argument: the host tests show that the envelope accepts the emulation and rejects every planted defect.
"""
import math

import numpy as np
import torch

from bf16_ref import EPS32, bf, dot_delta, prologue

U = EPS32
TINY = 2.0 ** -126          # smallest normal fp32: the absolute error of an operation whose result underflows
# expf / logf: the HIP math library documents 1 ulp for both; 2 is allowed (one spare for an implementation that is
# not the documented one, e.g. numpy's in the emulation).  One ulp is at most 2 u relative.
ULP_EXP = 2.0
ULP_LOG = 2.0
ULP_SQRT = 1.0              # sqrtf without fast-math: correctly rounded (0.5 ulp), 1 allowed


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# slots: a logical [rows, cols] operand inside a larger NaN-filled buffer
# ---------------------------------------------------------------------------------------------
class Slot(object):
    """fp32 [rows, cols] view at row `pre`, column `left` of a NaN-filled [pre + rows + post, ld] buffer; ld = left +
    cols + right rounded up to a multiple of 4, so with `left` a multiple of 4 every row of the view starts on 16 bytes
    (what bt_vec_ok asks for).  left = 5 gives a base 4 bytes off such a boundary."""

    def __init__(self, rows, cols, device, left=4, right=5, pre=2, post=3, ld=None):
        self.ld = _cdiv(left + cols + right, 4) * 4 if ld is None else ld
        self.buf = torch.full((pre + rows + post, self.ld), float("nan"), dtype=torch.float32, device=device)
        self.view = self.buf[pre:pre + rows, left:left + cols]
        self.box = (pre, pre + rows, left, left + cols)

    def set(self, t):
        self.view.copy_(t)
        return self.view

    def clear(self):
        self.buf.fill_(float("nan"))
        return self.view

    def outside_is_nan(self):
        keep = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        r0, r1, c0, c1 = self.box
        keep[r0:r1, c0:c1] = False
        return bool(torch.isnan(self.buf[keep]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


class Vec(object):
    """fp32 [n] view starting `off` floats into a NaN-filled buffer with `off` + 7 guard elements"""

    def __init__(self, n, device, off=4):
        self.buf = torch.full((off + n + 7,), float("nan"), dtype=torch.float32, device=device)
        self.view = self.buf[off:off + n]
        self.off, self.n = off, n

    def set(self, t):
        self.view.copy_(t)
        return self.view

    def clear(self):
        self.buf.fill_(float("nan"))
        return self.view

    def outside_is_nan(self):
        return bool(torch.isnan(self.buf[:self.off]).all() and torch.isnan(self.buf[self.off + self.n:]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


def ratio(got, want, tol, where=None):
    """(worst |got - want| / tol, number of elements outside tol); a non-finite `got` counts as outside.  where: the
    elements that are judged."""
    got = torch.as_tensor(got).double().cpu()
    want = torch.as_tensor(want).double().cpu()
    tol = torch.as_tensor(tol).double().cpu()
    err = (got - want).abs()
    bad = ~(err <= tol)                               # NaN compares false: counted
    r = err / tol.clamp_min(1e-300)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    if where is not None:
        where = torch.as_tensor(where).cpu()
        bad = bad & where
        r = torch.where(where, r, torch.zeros_like(r))
    return (float(r.max()) if r.numel() else 0.0), int(bad.sum())


# ---------------------------------------------------------------------------------------------
# softmax cross entropy
# ---------------------------------------------------------------------------------------------
def ce_rows_kernel(K, work_given):
    """the dispatch of yolat_softmax_ce: k_softmax_ce_rows + k_ce_final iff a scratch buffer is given and K <= 32,
    else the single-workgroup k_softmax_ce"""
    return bool(work_given) and K <= 32


def ce_workgroups(P):
    return _cdiv(P, 256)


def ce_depth(P, rows_kernel):
    """the number of fp32 additions a row's loss goes through on its way into the total (every one rounds once):
    rows kernel: 8 tree levels of 256, the thread's ceil(nwg / 1024) serial additions of k_ce_final, 10 tree levels;
    single workgroup: the thread's ceil(P / 1024) serial additions, 10 tree levels"""
    if rows_kernel:
        return 8 + _cdiv(ce_workgroups(P), 1024) + 10
    return _cdiv(P, 1024) + 10


def ce_families():
    return ["randn3", "equal", "offset1e4", "spread90", "sure50"]


def ce_inputs(P, K, family, seed):
    """(logits fp32 [P,K], labels int64 [P]) of an input family of the issue"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(P, K, generator=g) * 3
    y = torch.randint(0, K, (P,), generator=g)
    if family == "randn3":
        pass
    elif family == "equal":                     # all logits of a row equal
        z = z[:, :1].expand(P, K).contiguous()
    elif family == "offset1e4":                 # exp(1e4) overflows without the max subtraction
        z = z + 1e4
    elif family == "spread90":                  # +-90 about the row mean: expf(z - m) underflows to 0 on the low side
        sgn = torch.where(torch.rand(P, K, generator=g) < 0.5, -1.0, 1.0)
        sgn[:, 0], sgn[:, K - 1] = 1.0, -1.0
        z = z[:, :1] + 90.0 * sgn
        y = torch.where(torch.arange(P) % 2 == 0, torch.full_like(y, K - 1), y)      # label on an underflowed column
    elif family == "sure50":                    # row 3: the label logit is the maximum by 50: p_y rounds to 1
        r = min(3, P - 1)
        z[r, int(y[r])] = z[r].max() + 50.0
    else:
        raise ValueError(family)
    return z.float().contiguous(), y


def softmax_ce_ref(z32, labels, rows_kernel):
    """float64 loss = mean(lse - z_y), dl = (softmax - onehot) / P of fp32 logits, and the envelopes of an fp32
    implementation that subtracts the row maximum:
        t = fl(z - m) (|t| u absolute -> exp(t) relative), e = expf(t): rel_e = (|t| + 2 ULP_EXP) u
        s = sum e in any order: rel_s = (K - 1) u + sum_k p_k rel_e_k + K TINY / s   (TINY: a flushed expf)
        row = fl(fl(m + logf(s)) - z_y): rel_s + 2 ULP_LOG u |log s| + u |lse| + u |row|
        loss: sum tol_row / P + (depth + 2) u sum |row| / P   (depth additions, 1 / P and its product)
        dl = fl(fl(fl(e fl(1 / s)) - onehot) fl(1 / P)): (p (rel_e + rel_s + 2 u) + u |p - onehot| + TINY) / P + 2 u |dl|
    A label outside [0, K) poisons the loss (NaN); `good` marks the rows whose dl is defined.
    Returns dict(loss, tol_loss, dl, tol_dl, good)."""
    z = torch.as_tensor(z32).double().cpu()
    labels = torch.as_tensor(labels).cpu()
    P, K = z.shape
    good = (labels >= 0) & (labels < K)
    y = labels.clamp(0, K - 1)
    m = z.max(1).values
    t = z - m[:, None]
    e = torch.exp(t)
    s = e.sum(1)
    p = e / s[:, None]
    logs = torch.log(s)
    lse = m + logs
    row = lse - z.gather(1, y[:, None])[:, 0]
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0)
    dl = (p - onehot) / P
    rel_e = (t.abs() + 2 * ULP_EXP) * U
    rel_s = (K - 1) * U + (p * rel_e).sum(1) + K * TINY / s
    tol_row = rel_s + 2 * ULP_LOG * U * logs.abs() + U * lse.abs() + U * row.abs()
    depth = ce_depth(P, rows_kernel)
    loss = row.sum() / P if bool(good.all()) else torch.tensor(float("nan"), dtype=torch.float64)
    tol_loss = (tol_row.sum() + (depth + 2) * U * row.abs().sum()) / P
    tol_dl = (p * (rel_e + rel_s[:, None] + 2 * U) + U * (p - onehot).abs() + TINY) / P + 2 * U * dl.abs()
    return dict(loss=loss, tol_loss=tol_loss, dl=dl, tol_dl=tol_dl, good=good)


def _tree(red):
    """the fixed-order tree of the kernels over the last axis (a power of two): red[t] += red[t + s], s = n/2 .. 1"""
    red = red.copy()
    s = red.shape[-1] // 2
    while s > 0:
        red[..., :s] = red[..., :s] + red[..., s:2 * s]
        s //= 2
    return red[..., 0]


def emulate_softmax_ce(z32, labels, rows_kernel, defect=None):
    """(loss fp32 scalar, dl fp32 [P,K]) as the kernels compute them, in numpy fp32.  defect: None, "inv_p1" (1 / (P +
    1)), "no_max" (no max subtraction), "wrong_row" (the label column of the next row), "drop_partial" (the last
    workgroup's partial, or the last thread's in the single-workgroup kernel, left out of the final sum)."""
    f = np.float32
    z = np.asarray(z32, dtype=f)
    y_all = np.asarray(labels, dtype=np.int64)
    P, K = z.shape
    bad = (y_all < 0) | (y_all >= K)
    y = np.where(bad, 0, y_all)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        m = z.max(1) if defect != "no_max" else np.zeros(P, dtype=f)
        e = np.exp((z - m[:, None]).astype(f)).astype(f)
        s = np.zeros(P, dtype=f)
        for k in range(K):
            s = (s + e[:, k]).astype(f)
        src = z if defect != "wrong_row" else np.roll(z, -1, axis=0)
        row = ((m + np.log(s).astype(f)).astype(f) - src[np.arange(P), y]).astype(f)
        row = np.where(bad, f("nan"), row).astype(f)
        Pd = P + 1 if defect == "inv_p1" else P
        inv_p = f(1.0) / f(Pd)
        onehot = np.zeros((P, K), dtype=f)
        onehot[np.arange(P), y] = 1.0
        dl = (((e * (f(1.0) / s)[:, None]).astype(f) - onehot).astype(f) * inv_p).astype(f)
        if rows_kernel:
            nwg = _cdiv(P, 256)
            red = np.zeros(nwg * 256, dtype=f)
            red[:P] = row
            work = _tree(red.reshape(nwg, 256))
            if defect == "drop_partial":
                work = work[:-1]
            a = np.zeros(_cdiv(max(len(work), 1), 1024) * 1024, dtype=f)
            a[:len(work)] = work
            acc = np.zeros(1024, dtype=f)
            for c in a.reshape(-1, 1024):
                acc = (acc + c).astype(f)
            loss = f(_tree(acc)) / f(Pd)
        else:
            a = np.zeros(_cdiv(P, 1024) * 1024, dtype=f)
            a[:P] = row
            acc = np.zeros(1024, dtype=f)
            for c in a.reshape(-1, 1024):
                acc = (acc + c).astype(f)
            if defect == "drop_partial":
                acc[min(P, 1024) - 1] = 0.0
            loss = f(_tree(acc)) * inv_p
    return f(loss), dl


# ---------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale):
    """One torch.optim.Adam step in float64 from fp32 state, and per-element envelopes of k_adam:
        g' = g gs + wd p;  m' = m + (g' - m)(1 - b1);  v' = b2 v + (1 - b2) g'^2
        p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc = 1 - b^step
    lr, b1, b2, eps are the requested (Python float) values.  The entry point takes them as fp32, so each reaches the
    kernel within u relative: factor 1 on u b |.| below (1 - b inherits the ABSOLUTE error u b), and bc = 1 - b^step moves
    by step u b^step.  Roundings counted, statement by statement (a contraction into fma only removes one):
        g':  u |g gs| (if gs != 1) + u |wd p| + u |g'| (if wd != 0)
        m':  (1 - b1) dg + (2 (1 - b1) + b1) u |g' - m| + u |m'|
        v':  (1 - b2)(2 |g'| dg + dg^2) + u (2 b2 |v| + (2 (1 - b2) + b2) g'^2 + |v'|)
        r = sqrtf(v'): the interval [sqrt(v' - dv), sqrt(v' + dv)] + 2 ULP_SQRT u r
        den = fl(fl(r ibs) + eps), q = fl(m' / den), upd = fl(ss q), p' = fl(p - upd): one u each, ss and ibs within
        (dbc / bc (half of it for the square root) + 2 u) of their values
    and TINY wherever a result may underflow.  Returns dict(p, m, v, tol_p, tol_m, tol_v) in float64."""
    P, G, M, V = [torch.as_tensor(t).double().cpu() for t in (p, g, m, v)]
    b1, b2 = float(beta1), float(beta2)
    g1 = G * grad_scale
    gp = g1 + wd * P
    dg = torch.zeros_like(G)
    if grad_scale != 1.0:
        dg = dg + U * g1.abs()
    if wd != 0.0:
        dg = dg + U * (abs(wd) * P.abs() + gp.abs()) + TINY
    m2 = M + (gp - M) * (1 - b1)
    tm = (1 - b1) * dg + (2 * (1 - b1) + b1) * U * (gp - M).abs() + U * m2.abs() + TINY
    v2 = b2 * V + (1 - b2) * gp * gp
    tv = (1 - b2) * (2 * gp.abs() * dg + dg * dg) + U * (2 * b2 * V.abs() + (2 * (1 - b2) + b2) * gp * gp + v2.abs()) \
        + 4 * TINY
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    dbc1, dbc2 = step * U * b1 ** step, step * U * b2 ** step
    ss, ibs = lr / bc1, 1 / math.sqrt(bc2)
    dss, dibs = ss * (dbc1 / bc1 + 2 * U), ibs * (0.5 * dbc2 / bc2 + 2 * U)
    r = torch.sqrt(v2)
    dr = torch.sqrt(v2 + tv) - torch.sqrt((v2 - tv).clamp_min(0)) + 2 * ULP_SQRT * U * r
    den = r * ibs + eps
    dden = dr * (ibs + dibs) + r * dibs + U * r * ibs + U * eps + U * den
    q = m2 / den
    dq = tm / (den - dden) + m2.abs() * dden / (den * (den - dden)) + U * q.abs() + TINY
    upd = ss * q
    dupd = dss * q.abs() + (ss + dss) * dq + U * upd.abs() + TINY
    p2 = P - upd
    tp = dupd + U * p2.abs() + TINY
    return dict(p=p2, m=m2, v=v2, tol_p=tp, tol_m=tm, tol_v=tv)


def emulate_adam(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, defect=None):
    """k_adam and the host part of yolat_adam_step in numpy fp32.  defect: None, "v_g" (v updated with g, not g^2),
    "eps_in_sqrt", "bc_step_m1" (bias corrections of step - 1), "no_grad_scale", "wd_always" (a weight decay of 1e-5
    applied although 0 was asked for).  Returns (p, m, v) fp32."""
    f = np.float32
    p, g, m, v = [np.asarray(t, dtype=f) for t in (p, g, m, v)]
    lr, b1, b2, eps, wd, gs = f(lr), f(beta1), f(beta2), f(eps), f(wd), f(grad_scale)
    st = step - 1 if defect == "bc_step_m1" else step
    with np.errstate(all="ignore"):
        bc1 = 1.0 - float(b1) ** st
        bc2 = 1.0 - float(b2) ** st
        step_size = f(np.float64(lr) / np.float64(bc1))
        inv_bc2_sqrt = f(np.float64(1.0) / np.sqrt(np.float64(bc2)))
        gi = g if defect == "no_grad_scale" else (g * gs).astype(f)
        if defect == "wd_always" and wd == 0:
            wd = f(1e-5)
        if wd != 0:
            gi = (np.float64(wd) * p.astype(np.float64) + gi.astype(np.float64)).astype(f)         # fmaf: one rounding
        mi = (m + ((gi - m).astype(f) * (f(1) - b1)).astype(f)).astype(f)
        gg = ((f(1) - b2) * gi).astype(f)
        if defect != "v_g":
            gg = (gg * gi).astype(f)
        vi = ((v * b2).astype(f) + gg).astype(f)
        if defect == "eps_in_sqrt":
            denom = (np.sqrt((vi + eps).astype(f)).astype(f) * inv_bc2_sqrt).astype(f)
        else:
            denom = ((np.sqrt(vi).astype(f) * inv_bc2_sqrt).astype(f) + eps).astype(f)
        pi = (p - (step_size * (mi / denom).astype(f)).astype(f)).astype(f)
    return pi, mi, vi


ADAM_FAMILIES = ("randn", "zero", "tiny", "huge", "p0")


def adam_inputs(n, seed):
    """(p, g, m, v) fp32 [n] and the family index of every element: element i belongs to family i % 5 —
    randn state; g = m = v = 0; |g| = 1e-30 on m = v = 0; |g| = 1e15; p = 0."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.randn(n, generator=gen) ** 2 * 0.5
    fam = torch.arange(n) % 5
    sgn = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    zero, tiny, huge, p0 = fam == 1, fam == 2, fam == 3, fam == 4
    g = torch.where(zero, torch.zeros(n), g)
    g = torch.where(tiny, 1e-30 * sgn, g)
    g = torch.where(huge, 1e15 * sgn, g)
    m = torch.where(zero | tiny, torch.zeros(n), m)
    v = torch.where(zero | tiny, torch.zeros(n), v)
    p = torch.where(p0, torch.zeros(n), p)
    return p.float(), g.float(), m.float(), v.float(), fam


# ---------------------------------------------------------------------------------------------
# dropout: the documented counter-based generator
# ---------------------------------------------------------------------------------------------
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def hash32(seed, idx):
    """top 32 bits of the splitmix64 finaliser on seed + 0x9E3779B97F4A7C15 (idx + 1), uint64 arithmetic with wrap-around"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.full(idx.shape, seed % (1 << 64), dtype=np.uint64) + _GOLDEN * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def dropout_thresh(p):
    """min(floor(p 2^32), 2^32 - 1), p taken as the fp32 value"""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def dropout_inv_keep(p):
    """1.f / (1.f - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_mask(seed, M, C, p, defect=None):
    """uint8 [M, C]: keep[r, c] = hash32(seed, r C + c) >= thresh.  defect: "gt" (>), "transposed" (index c M + r)"""
    r, c = np.meshgrid(np.arange(M, dtype=np.uint64), np.arange(C, dtype=np.uint64), indexing="ij")
    idx = c * np.uint64(M) + r if defect == "transposed" else r * np.uint64(C) + c
    h = hash32(seed, idx)
    t = np.uint32(dropout_thresh(p))
    return (h > t if defect == "gt" else h >= t).astype(np.uint8)


def dropout_edge_p(seed, n):
    """(p, idx): an fp32 p in [0.5, 0.95) whose threshold p 2^32 EQUALS hash32(seed, idx) for a position idx < n — the
    one element that `>=` keeps and `>` drops.  p 2^32 has 24 significant bits, so the hash needs 8 low zero bits."""
    h = hash32(seed, np.arange(n, dtype=np.uint64))
    ok = np.nonzero(((h & np.uint32(0xFF)) == 0) & (h >= np.uint32(1 << 31)) & (h < np.uint32(int(0.95 * 2 ** 32))))[0]
    if len(ok) == 0:
        raise ValueError("no position of %d hashes onto an fp32 threshold with seed %d" % (n, seed))
    i = int(ok[0])
    p = np.float32(float(h[i]) / 4294967296.0)
    assert dropout_thresh(p) == int(h[i])
    return float(p), i


def dropout_fwd_ref(Y, scale, shift, relu, p, seed, defect=None):
    """(mask uint8 [M,C], Z fp32 [M,C]) numpy.  v = fma(y, scale, shift) is evaluated in float64 and cast: exact for the
    grid inputs of bf16_ref (the caller asserts it), so Z == fp32(v fp32(1 / (1 - p))) is an equality.  defect: those of
    dropout_mask, and "scale_dropped" (inv_keep applied to the dropped elements too)."""
    y = np.asarray(Y, dtype=np.float64)
    M, C = y.shape
    v = y if scale is None else y * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    v = v.astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0))
    mask = dropout_mask(seed, M, C, p, defect)
    scaled = (v * dropout_inv_keep(p)).astype(np.float32)
    Z = scaled if defect == "scale_dropped" else np.where(mask != 0, scaled, np.float32(0)).astype(np.float32)
    return mask, Z


def dropout_bwd_ref(dZ, mask, p):
    dz = np.asarray(dZ, dtype=np.float32)
    return np.where(np.asarray(mask).reshape(dz.shape) != 0, (dz * dropout_inv_keep(p)).astype(np.float32),
                    np.float32(0)).astype(np.float32)


def keep_count_ok(kept, n, p):
    """the kept count lies within 5 sqrt(n p (1 - p)) of n (1 - p)"""
    return abs(kept - n * (1 - p)) <= 5 * math.sqrt(n * p * (1 - p))


# ---------------------------------------------------------------------------------------------
# bf16_dense GEMMs
# ---------------------------------------------------------------------------------------------
def bt_activation(M, K, seed):
    """fp32 [M,K]: k / 4096, |k| <= 2^14 — up to 15 significant bits, so NOT bfloat16 values, and exact ties of the
    rounding to 8 bits are frequent.  With bf16_ref.grid_scale_shift, a scale + shift = (k j + 512 m) / 32768 with
    |k j + 512 m| <= 12 * 2^14 + 512 * 64 < 2^24: exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(1 << 14), (1 << 14) + 1, (M, K), generator=g).float() / 4096.0


def bt_weight(N, K, seed):
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * 0.05


def bt_operand(a, scale, shift, relu):
    """float64 bf(pro(a)): the prologue in float64 (exact on the grid), then ONE rounding to nearest even"""
    if scale is None:
        return bf(a.double())
    return bf(prologue(a, scale, shift, relu))


def bt_gemm_ref(X, Y, k_red, bias=None, base=None):
    """want = X . Y^T (+ bias) (+ base) for float64 operands X [m, k], Y [n, k] that are already bfloat16 values, and
    tol = dot_delta(|X| . |Y|^T + |bias|, k_red) + u |want| (+ u (|base| + |want|) for the accumulating store).
    dot_delta carries the factor 2 for the matrix core's undocumented internal order (bf16_ref); u |want| is the store of
    the fp32 accumulator's final value."""
    want = X @ Y.t()
    mag = X.abs() @ Y.abs().t()
    if bias is not None:
        want = want + bias.double()
        mag = mag + bias.double().abs()
    tol = dot_delta(mag, k_red) + U * want.abs()
    if base is not None:
        want = want + base.double()
        tol = tol + U * (base.double().abs() + want.abs())
    return want, tol


def bt_dw_plan(M, N, K):
    """(S, kper) of the weight gradient's split-K plan (bt_dw_plan of bf16_train.hip, restated): ceil(512 / tiles) splits
    wanted, at most ceil(M / 256), every split a multiple of 32 rows"""
    tiles = _cdiv(N, 64) * _cdiv(K, 64)
    s = max(1, min(_cdiv(512, tiles), _cdiv(M, 256)))
    kper = _cdiv(_cdiv(M, s), 32) * 32
    return _cdiv(M, kper), kper


def bt_dw_work_elems(M, N, K):
    S, _ = bt_dw_plan(M, N, K)
    return (S * N * K if S > 1 else 0) + _cdiv(M, 32) * N + 64


def bt_db_ref(dY):
    """float64 column sums of the fp32 dY and the bound (32 + ceil(M / 32) + 2) u sum |dY|: 32 serial additions per chunk
    (k_bt_colsum), ceil(M / 32) serial additions of the chunks (k_bt_reduce), 2 spare"""
    d = dY.double()
    M = d.shape[0]
    return d.sum(0), (32 + _cdiv(M, 32) + 2) * U * d.abs().sum(0)


def bt_stats_ref(y, rows=32):
    """(sum, M2 about the group mean) per `rows`-row group (last group: cnt = M % rows) of the STORED values y [M, N]
    (float64 of fp32) and the envelopes of k_bt_gemm's statistics epilogue:
        sum:  cnt - 1 additions in a fixed tree + the lane-half exchange: (cnt + 2) u sum |y|
        mean' = fl(sum' / cnt): |dmu| <= tol_sum / cnt + u |mu|
        M2' = sum fl(fl(y - mean')^2): sum (y - mean')^2 = M2 + cnt dmu^2 exactly (sum (y - mu) = 0); the subtraction
              (twice, through the square), the square and cnt - 1 additions round once each, one spare for second order:
              cnt dmu^2 + (cnt + 3) u (M2 + cnt dmu^2)
    Returns (sum [G,N], m2 [G,N], tol_sum, tol_m2)."""
    M, N = y.shape
    G = _cdiv(M, rows)
    z = torch.zeros(G * rows - M, N, dtype=torch.float64, device=y.device)
    yp = torch.cat([y.double(), z]).view(G, rows, N)
    ok = torch.cat([torch.ones(M, 1, dtype=torch.float64, device=y.device), z[:, :1]]).view(G, rows, 1)
    cnt = ok.sum(1)
    s = yp.sum(1)
    mu = s / cnt
    d = (yp - mu[:, None, :]) * ok
    m2 = (d * d).sum(1)
    tol_s = (cnt + 2) * U * yp.abs().sum(1)
    dmu = tol_s / cnt + U * mu.abs()
    tol_m2 = cnt * dmu * dmu + (cnt + 3) * U * (m2 + cnt * dmu * dmu)
    return s, m2, tol_s, tol_m2


def _round_bf16(x32, mode):
    """fp32 -> the fp32 value of its bfloat16 rounding.  mode: "rne" (the contract), "trunc", "away" (ties away from 0)"""
    if mode == "rne":
        return x32.to(torch.bfloat16).float()
    bits = x32.contiguous().view(torch.int32)
    if mode == "trunc":
        return (bits & -65536).view(torch.float32)
    if mode == "away":                       # sign-magnitude: adding half a spacing to the raw bits grows the magnitude
        return ((bits + 0x8000) & -65536).view(torch.float32)
    raise ValueError(mode)


def emulate_bt_operand(a32, scale, shift, relu, mode="rne", pro_after_round=False):
    """bt_pack8 in fp32 on the CPU: fma prologue (float64 then cast: one rounding), ReLU, rounding.  pro_after_round: the
    operand is rounded first and the prologue's result is used as it is."""
    a = a32.float()
    if scale is None:
        return _round_bf16(a, mode)
    if pro_after_round:
        a = _round_bf16(a, mode)
    z = (a.double() * scale.double() + shift.double()).float()
    if relu:
        z = torch.relu(z)
    return z if pro_after_round else _round_bf16(z, mode)


def emulate_bt_gemm(X, Y, bias=None, splits=None, dup_last_row=False, skip_last_tile=False):
    """fp32 X . Y^T of already-rounded operands X [m, k], Y [n, k].  splits: [(kb, ke)] of the split-K form, whose fp32
    partials are added in order (k_bt_reduce).  skip_last_tile: the last split stops 32 k short.  dup_last_row: the last
    row of the output is a copy of the one before (a tile-edge bug)."""
    k = X.shape[1]
    splits = [(0, k)] if splits is None else list(splits)
    if skip_last_tile:
        kb, ke = splits[-1]
        splits[-1] = (kb, max(kb, ke - 32))
    acc = None
    for kb, ke in splits:
        part = X[:, kb:ke] @ Y[:, kb:ke].t()
        acc = part if acc is None else acc + part
    if bias is not None:
        acc = acc + bias
    if dup_last_row and acc.shape[0] >= 2:
        acc = acc.clone()
        acc[-1] = acc[-2]
    return acc


def bt_splits(M, N, K):
    S, kper = bt_dw_plan(M, N, K)
    return [(s * kper, min(M, (s + 1) * kper)) for s in range(S)]


# ---------------------------------------------------------------------------------------------
# the cases of the GPU tests (the host tests run the emulations over the same ones)
# ---------------------------------------------------------------------------------------------
# (P, K) with a scratch buffer: 1 row; K = 1, 2; P around one 256-row workgroup; K at and below the 32 registers of the
# rows kernel; 1026 workgroups, so k_ce_final's stride loop takes a second trip
CE_ROWS_SHAPES = [(1, 1), (1, 2), (255, 17), (256, 32), (257, 31), (3000, 22), (262144 + 300, 5)]
# (P, K, scratch given): the single-workgroup kernel — K > 32 (one and two trips of the 1024-thread row loop), no scratch
CE_SINGLE_SHAPES = [(257, 33, True), (1025, 40, True), (700, 17, False)]
CE_FAMILY_SHAPES = [(257, 31), (257, 33)]

ADAM_HP = dict(lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_N = [1, 255, 257, 100003, 4096 * 256 + 1]                  # the last: one element in the grid-stride second trip
ADAM_GRID = [(0.0, 1.0, 1), (1e-5, 1.0 / 3.0, 2), (0.0, 0.125, 1000), (1e-5, 1.0, 10 ** 6), (1e-5, 1.0 / 3.0, 1)]   # (wd, gs, step)

DROP_SHAPES = [(1, 64), (5, 7), (333, 64), (1000, 1024)]
DROP_P = [0.0, 0.1, 0.5, 0.9]
DROP_SEEDS = (20240611, 977)

# (M, K, N, prologue, bias, stats)
BT_FWD_CASES = [(1, 32, 1, "none", True, True), (31, 32, 33, "affine", True, True), (33, 64, 65, "relu", False, True),
                (64, 96, 64, "none", True, False), (65, 128, 127, "relu", True, True),
                (129, 2304, 72, "affine", False, False), (300, 512, 130, "relu", True, True)]
BT_WT_CASES = [(1, 32, 8), (33, 64, 72), (65, 96, 136), (200, 512, 2304)]
# (M, N, K, prologue, db, split-K expected)
BT_DW_CASES = [(1, 8, 8, "none", True, False), (31, 72, 40, "relu", False, False), (33, 64, 64, "none", True, False),
               (255, 72, 40, "relu", True, False), (257, 72, 40, "relu", True, True), (257, 64, 64, "none", False, True),
               (1007, 256, 512, "none", True, True), (8000, 128, 128, "relu", True, True)]
