"""float64 reference helpers for the bf16-STORAGE training ops (tests/test_gpu_bf16_storage_ops.py).  CPU only: torch and
numpy, no import of the extension (tests/test_bf16_ref_host.py checks every claim made here).

The kernels of this mode (include/yolat_hip.h, "Training with bfloat16 STORAGE") accumulate in fp32 and round to
nearest even when they store bfloat16.  A reference value therefore has two error terms: `delta`, the fp32 accumulation
bound formed from the operand MAGNITUDES of the op, and half a bfloat16 spacing of the stored value.  store_envelope
adds the two per element.  Nothing here is scaled by a tensor maximum.

Inputs that go through a kernel's (scale, shift) prologue are drawn from a grid on which fma(a, scale, shift) is exact in
fp32, so the reference has no rounding ambiguity of its own:
    activation k/64 (|k| <= 256), scale j/8 (j in 4..12), shift m/64 (|m| <= 64)
    a*scale + shift = (k j + 8 m) / 512 with |k j + 8 m| <= 3584 < 2^24
"""
import numpy as np
import torch

EPS32 = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
KINK = 1e-4                 # |z| above this: the ReLU mask is the same in fp32 and fp64 (test_gpu_ops.py's `sure`)
KINK_SHARE = 1e-3           # at most this share of the elements may sit on the kink


# ---------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """The spacing of bfloat16 (8 significant bits) at |v|, float64: 2^(floor(log2 |v|) - 7), and the spacing of the
    smallest normal binade (2^-133) at zero and below it.  No pow / exp2: |v| = m 2^e with m in [0.5, 1) (frexp), the
    quotient |v| / m = 2^e is exact, and so is its scaling by 2^-8."""
    a = torch.as_tensor(v, dtype=torch.float64).abs()
    m, _ = torch.frexp(a)
    safe = a > 0
    u = torch.where(safe, a, torch.ones_like(a)) / torch.where(safe, m, torch.ones_like(a)) * 2.0 ** -8
    return torch.where(safe, u, torch.zeros_like(a)).clamp(min=2.0 ** -133)


def bf(t):
    """Round to nearest even to bfloat16, returned as float64.  fp32 / bf16 input: torch's conversion; float64 input: the
    same rounding done in float64 (torch would go through fp32 first and round twice)."""
    t = torch.as_tensor(t)
    if t.dtype != torch.float64:
        return t.to(torch.bfloat16).double()
    u = ulp_bf16(t)
    return torch.round(t / u) * u                      # torch.round: halves to even; t / u is exact (u a power of two)


def truncate_bf16(t32):
    """fp32 -> bfloat16 by dropping the low 16 bits (what a store WITHOUT rounding does), returned as bfloat16."""
    bits = t32.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def store_envelope(want, delta):
    """Elementwise tolerance of a value accumulated in fp32 (within `delta` of `want`) and then stored as bfloat16 with
    round to nearest: the accumulator lies in [want - delta, want + delta], the store moves it by at most half a
    spacing at that magnitude."""
    want = torch.as_tensor(want, dtype=torch.float64)
    delta = torch.as_tensor(delta, dtype=torch.float64)
    return 0.5 * ulp_bf16(want.abs() + delta) + delta


def dot_delta(abs_products, K):
    """fp32 accumulation bound of a length-K dot product (+ bias): 2 (K + 2) 2^-24 (|a| . |w| + |bias|), `abs_products`
    being that magnitude sum.  (K + 2) 2^-24 is the classical bound for K additions in any order + the bias; the factor
    2 is there because the matrix core's internal accumulation order and intermediate width are not documented."""
    return 2.0 * (K + 2) * EPS32 * abs_products


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def grid_activation(M, K, seed):
    """[M,K] bfloat16 activations k/64, |k| <= 256 (exact in bfloat16: |k| <= 255 has at most 8 bits, 256 = 2^8)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-256, 257, (M, K), generator=g)
    return (k.float() / 64.0).to(torch.bfloat16)


def grid_scale_shift(K, seed):
    """(scale, shift) fp32 [K]: scale j/8 with j in 4..12, shift m/64 with |m| <= 64"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.randint(4, 13, (K,), generator=g).float() / 8.0
    shift = torch.randint(-64, 65, (K,), generator=g).float() / 64.0
    return scale, shift


def prologue(a, scale, shift, relu):
    """float64 max(a*scale + shift, floor): floor 0 with ReLU, -inf without"""
    z = a.double() * scale.double() + shift.double()
    return torch.relu(z) if relu else z


def prologue_is_exact_in_fp32(a, scale, shift):
    """the fp32 result of a*scale + shift (two roundings at worst) equals the float64 one"""
    z32 = a.float() * scale + shift
    return bool(torch.equal(z32.double(), a.double() * scale.double() + shift.double()))


def bn_bwd_inputs(M, C, seed):
    """Inputs of a BatchNorm(train) + ReLU backward with REAL statistics: Y, dZ [M,C] bfloat16; save_mean, save_invstd,
    scale = gamma invstd, shift = beta - mean scale as the fp32 vectors the kernel is given.  |beta| >= 1/16 keeps a
    single-row batch (xhat = 0, z = beta) off the ReLU kink."""
    g = torch.Generator().manual_seed(seed)
    Y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    dZ = torch.randn(M, C, generator=g).to(torch.bfloat16)
    y = Y.double()
    mean = y.mean(0)
    invstd = 1.0 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, generator=g).double() + 0.5
    beta = (torch.rand(C, generator=g).double() * 0.5 + 0.0625) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    mean32, invstd32 = mean.float(), invstd.float()
    scale32 = (gamma * invstd).float()
    shift32 = (beta - mean * gamma * invstd).float()
    return Y, dZ, mean32, invstd32, scale32, shift32


def kink_share(Y, scale, shift):
    """share of the elements whose pre-activation z = Y scale + shift lies within KINK of zero (float64, row chunks)"""
    n = 0
    for r0 in range(0, Y.shape[0], 65536):
        z = Y[r0:r0 + 65536].double() * scale.double() + shift.double()
        n += int((z.abs() <= KINK).sum())
    return n / float(max(Y.numel(), 1))


def bn_relu_bwd_ref(dZ, Y, mean, invstd, scale, shift, relu, coef=None):
    """float64 restatement of the backward of Z = relu(BN_train(Y)) (test_gpu_ops.py::test_bn_apply_edge_sums_...):
        dY = scale (g - c1 - xhat c2),  g = dZ [z > 0],  z = Y scale + shift,  xhat = (Y - mean) invstd,
        (c1, c2) = (sum g, sum g xhat) / M   unless `coef` [2C] = (c1 | c2) is given.
    Returns a dict: dY, dgamma (= sum g xhat), dbeta (= sum g), c1, c2, g, xhat, sure (|z| > KINK)."""
    dZ, Y = dZ.double(), Y.double()
    mean, invstd, scale, shift = mean.double(), invstd.double(), scale.double(), shift.double()
    M, C = Y.shape
    z = Y * scale + shift
    sure = (z.abs() > KINK) if relu else torch.ones_like(z, dtype=torch.bool)
    g = dZ * (z > 0) if relu else dZ
    xhat = (Y - mean) * invstd
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    if coef is None:
        c1, c2 = s1 / M, s2 / M
    else:
        c1, c2 = coef[:C].double(), coef[C:].double()
    dY = scale * (g - c1 - xhat * c2)
    return dict(dY=dY, dgamma=s2, dbeta=s1, c1=c1, c2=c2, g=g, xhat=xhat, sure=sure)


# ---------------------------------------------------------------------------------------------
# graphs: (src, dst) int64 numpy arrays, in no particular edge order
# ---------------------------------------------------------------------------------------------
HUB_IN, HUB_OUT, QUIET = 1, 2, 130


def uniform(N, E, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, N, E).astype(np.int64), rng.integers(0, N, E).astype(np.int64)


def hub(N, E, deg, seed=0):
    """node HUB_IN holds exactly `deg` in-edges (a CSR segment over deg/64 sixty-four-row tiles), node HUB_OUT exactly
    `deg` out-edges, the QUIET nodes N-1-QUIET .. N-2 have no in-edge and the last node has no edge at all; the other
    E - 2 deg edges are uniform over what is left."""
    if N < QUIET + 10 or E < 2 * deg:
        raise ValueError("hub(%d, %d, %d): needs N >= %d and E >= 2 deg" % (N, E, deg, QUIET + 10))
    rng = np.random.default_rng(seed)
    n_dst = N - 1 - QUIET                                   # destinations: nodes 0 .. n_dst - 1
    src_pool = np.array([n for n in range(N - 1) if n != HUB_OUT], dtype=np.int64)
    dst_pool = np.array([n for n in range(n_dst) if n != HUB_IN], dtype=np.int64)
    rest = E - 2 * deg
    src = np.concatenate([rng.choice(src_pool, deg), np.full(deg, HUB_OUT, dtype=np.int64), rng.choice(src_pool, rest)])
    dst = np.concatenate([np.full(deg, HUB_IN, dtype=np.int64), rng.choice(dst_pool, deg), rng.choice(dst_pool, rest)])
    order = rng.permutation(E)
    return src[order].astype(np.int64), dst[order].astype(np.int64)


def chain(N):
    """node i receives its one edge from node i - 1 (cyclic): in-degree exactly 1 everywhere, E = N"""
    dst = np.arange(N, dtype=np.int64)
    return (dst - 1) % N, dst


def in_degree(dst, N):
    return np.bincount(dst, minlength=N)


def csr_mean_bwd_ref(d_out, dst, N):
    """float64 gradient of the mean aggregation w.r.t. the message of every edge: d_out[dst] / max(deg[dst], 1);
    dst: int64 tensor [E] (any edge order — the result follows it)"""
    deg = torch.bincount(dst, minlength=N).clamp_min(1).double()
    return d_out.double()[dst] / deg[dst][:, None]


def csr_mean_ref(h, dst, N):
    """float64 (mean over the in-edges of every node [N,C], sum of magnitudes [N,C], in-degree [N]) of rows h [E,C]"""
    C = h.shape[1]
    s = torch.zeros(N, C, dtype=torch.float64, device=h.device).index_add_(0, dst, h.double())
    mag = torch.zeros(N, C, dtype=torch.float64, device=h.device).index_add_(0, dst, h.double().abs())
    deg = torch.bincount(dst, minlength=N).double()
    return s / deg.clamp_min(1)[:, None], mag, deg


# ---------------------------------------------------------------------------------------------
# fp32 emulation of yolat_linear_fwd_h (host test: the envelope accepts it, and rejects two wrong stores)
# ---------------------------------------------------------------------------------------------
def emulate_linear_fwd_h(A, scale, shift, relu, W, bias, store="nearest", dup_last_row=False):
    """The kernel's arithmetic in fp32 on the CPU: prologue (fp32), re-round to bfloat16, fp32 GEMM against the
    bfloat16-rounded weight, bias, store.  store: "nearest" (the contract) or "truncate".  dup_last_row: the last row of
    the last 64-row tile comes out as a copy of the row before it (a tile-edge bug)."""
    a = A.float()
    if scale is not None:
        a = a * scale + shift
        if relu:
            a = torch.relu(a)
        a = a.to(torch.bfloat16).float()
    acc = a @ W.to(torch.bfloat16).float().t()
    if bias is not None:
        acc = acc + bias
    if dup_last_row and acc.shape[0] >= 2:
        acc = acc.clone()
        acc[-1] = acc[-2]
    return acc.to(torch.bfloat16) if store == "nearest" else truncate_bf16(acc)


def linear_fwd_ref(A, scale, shift, relu, W, bias):
    """(want, delta) of Y = bf(pro(A)) . bf(W)^T + bias in float64; delta = dot_delta of the operand magnitudes"""
    a = A.double()
    if scale is not None:
        a = bf(prologue(A, scale, shift, relu))
    wb = bf(W)
    b = bias.double() if bias is not None else torch.zeros(W.shape[0], dtype=torch.float64, device=W.device)
    want = a @ wb.t() + b
    mag = a.abs() @ wb.abs().t() + b.abs()
    return want, dot_delta(mag, A.shape[1])


def group_stats_ref(v, dv, rows=32):
    """(sum, M2 about the group mean) per `rows`-row group of v [M,N] float64 (last group short) and their tolerances for
    an fp32 implementation whose values are within dv of v:
        sum:  sum_r dv_r + (rows + 1) 2^-24 sum_r |v_r|                      (the values' error + rows fp32 additions)
        M2:   with mu' = fl(sum' / cnt), |dmu| <= tol_sum / cnt + 2^-24 |mu|:
              (v' - mu')^2 - (v - mu)^2 = 2 (v - mu)(e - dmu) + (e - dmu)^2 and sum_r (v_r - mu) = 0, so
              |dM2| <= 2 sum_r |v_r - mu| dv_r + sum_r (dv_r + |dmu|)^2 + (rows + 4) 2^-24 M2
              (last term: the subtraction, the square and the rows additions, each rounded once, first order)
    Returns (sum [G,N], m2 [G,N], tol_sum, tol_m2)."""
    M, N = v.shape
    G = (M + rows - 1) // rows
    pad = G * rows - M
    z = torch.zeros(pad, N, dtype=torch.float64, device=v.device)
    vp = torch.cat([v, z]).view(G, rows, N)
    dp = torch.cat([dv, z]).view(G, rows, N)
    ok = torch.cat([torch.ones(M, 1, dtype=torch.float64, device=v.device), z[:, :1]]).view(G, rows, 1)
    cnt = ok.sum(1)
    s = vp.sum(1)
    mu = s / cnt
    d = (vp - mu[:, None, :]) * ok
    m2 = (d * d).sum(1)
    tol_s = dp.sum(1) + (rows + 1) * EPS32 * vp.abs().sum(1)
    dmu = tol_s / cnt + EPS32 * mu.abs()
    tol_m2 = 2.0 * (d.abs() * dp).sum(1) + (((dp + dmu[:, None, :]) * ok) ** 2).sum(1) + (rows + 4) * EPS32 * m2
    return s, m2, tol_s, tol_m2
