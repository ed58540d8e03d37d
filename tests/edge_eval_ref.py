"""float64 reference, per-element envelopes and fp32 emulations of the fused EVAL edge stage — factorised edge MLP, mean
aggregation, root row — in its fp32 forms (csrc/edge.hip: k_edge_uv_mlp2_mean<1|4, NEXT>, k_edge_mt_uv_mlp2_mean,
k_edge_uv_mlp2_mean_ws<FOLD, X6>, and the message kernel k_edge_uv_mlp2) and its bf16-storage forms (csrc/edge_chain.hip:
k_edge_uv_mlp2_mean_h<1|4>, k_edge_chain_h).  CPU only: torch and numpy, no import of the extension.
tests/test_edge_eval_ref_host.py checks every claim made here; tests/test_gpu_edge_eval_elements.py holds the kernels to
these envelopes.

    h1 = relu(((U[dst] + V[src] + attr . Wc4^T) + b1) s1 + t1)      m = relu((h1 . W2^T + b2) s2 + t2)
    out = root + sum m / max(deg, 1)

on CSR-ordered edges, in both argument forms of the entry: unfolded (b1, s1, t1, b2, s2, t2) and folded (b1 = s1 = b2 =
None: ops.fold_factorised_layer moved them into UV, Wc4 and t2).

Every tolerance is per element, formed from u = 2^-24 (bf16: the spacing of the stored value) and the magnitudes that
element's arithmetic goes through, following the kernel source; nothing is scaled by a tensor maximum and no share of the
outputs is exempt.  The references are torch code that runs where its operands live (the GPU tests evaluate them in
float64 on the device).  The emulations are numpy / torch fp32 on the CPU.  They do not model the software pipeline; they
model what decides the result: the order of the operations of a message, CSR-order run sums cut into 64-row passes with a
carried partial sum and count, and mul_rn(sum, 1 / cnt) + root.  Each takes a `defect`; the host tests show that every
envelope accepts its clean emulation on every graph of EDGE_GRAPHS and rejects every planted defect.

Not covered: the `npt2` branch of yl_edge_tile_npt (two passes per tile on big graphs) needs N >= 131072 with the tile
variant forced, which the product never does (E >= 131072 goes to the wave-specialised kernel); it is left out.
"""
import numpy as np
import torch

import bf16_ref as br
import graph_ref as gr
from graph_ref import SLACK, U, csr_of, fma32, has_full_mantissa, mean_tol, randn32, run_sum_tol   # noqa: F401 (handed on)

C = 64
PASS = 64                   # rows of a pass of the tile and wave-specialised kernels
C2 = 2                      # the `c` of the (64 + c) u bound of layer 2: the products, should the matrix core round them
X6_DROP = 2.0 ** -21 + 2.0 ** -30
CLOSED = (5, 40)            # output columns with t2 = -50: every message is 0 there
ZERO_K = 17                 # hidden channel whose column of W2 is zero
F32 = np.float32


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# the three host formulas, restated (edge.hip: yl_edge_tile_npt, the ws chunk; edge_chain.hip: yl_edge_chain_bf16)
# ---------------------------------------------------------------------------------------------
def edge_tile_npt(N, E):
    if E <= 0:
        return 64
    npt = (56 * N) // E
    npt2 = min((112 * N) // E, 16)
    if npt2 >= 2 * npt - 2 and N // max(npt2, 1) >= 8192:
        npt = npt2
    return max(1, min(npt, 64))


def tile_layout(N, E):
    """dict(npt, NG, tiles) of the node-tile kernels"""
    npt = edge_tile_npt(N, E)
    return dict(npt=npt, NG=1 if npt <= 16 else 4, tiles=_cdiv(N, npt))


def ws_layout(E):
    """dict(chunk, grid) of k_edge_uv_mlp2_mean_ws: chunk = roundup64(ceil(E / 512)); None below one full pass"""
    if E < 64:
        return None
    chunk = max(64, _cdiv(_cdiv(E, 512), 64) * 64)
    return dict(chunk=chunk, grid=_cdiv(E, chunk))


def chain_layout(E):
    """dict(chunk, grid) of k_edge_chain_h: two streams of chunk = roundup16(ceil(E / 6144)) edges per wave, four waves
    per workgroup; None below E = 16"""
    if E < 16:
        return None
    chunk = max(16, _cdiv(_cdiv(E, 8 * 768), 16) * 16)
    need = _cdiv(E, 2 * chunk)
    return dict(chunk=chunk, grid=max(1, _cdiv(need, 4)))


# ---------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------
def gaps(seed=8):
    """(src, dst) int64, N = 200, E = 90: in-edges only into nodes 70..129, ten of those (seeded) have none, the other
    fifty have at least one; 70 empty nodes in front and 70 behind; sources anywhere; shuffled edge order"""
    rng = np.random.default_rng(seed)
    targets = np.sort(rng.permutation(np.arange(70, 130))[:50])
    dst = np.concatenate([targets, rng.choice(targets, 40)])
    src = rng.integers(0, 200, 90)
    order = rng.permutation(90)
    return src[order].astype(np.int64), dst[order].astype(np.int64)


U50_SEEDS = {63: 63, 64: 64, 65: 66, 127: 132, 128: 128, 129: 135}    # E > 64: rows 63 and 64 of the CSR order share a node


def _u50(E):
    return lambda: (50,) + br.uniform(50, E, seed=U50_SEEDS[E])


def _multi(N, E, kind):
    return lambda: (N,) + gr.bn_csr_graph(N, E, kind)


# name -> () -> (N, src, dst); the comment says what the entry reaches (EXPECT holds the numbers, the host test checks them)
EDGE_GRAPHS = dict(gr.GRAPHS)
# ladder    npt 3, NG 1, 15 tiles, the last partial; every in-degree 0..40; tiles of one and of two passes; 13 ws
#           workgroups, the last pass 52 rows
# hub65 / hub150 / hub1000   npt 8; one node over 2, 3 and 16 passes: the ws carry goes through both carry_s slots, and ws
#           workgroups whose whole chunk lies inside the hub return without writing
# chain257  npt 56, NG 4, the last tile 33 nodes; ws passes of 64 one-edge nodes: four nodes per aggregation thread, only
#           the first with its f_out row prefetched
# tiny      one NG = 4 tile; E < 64: the ws variants refuse; E < 16: the chained bf16 kernel too
EDGE_GRAPHS.update({
    # in-edges only into nodes 70..129: npt 64; ec_bound's c <= 0 and c >= E, "the last wave's range ends at N"
    "gaps": lambda: (200,) + gaps(),
    # the ws minimum of one full pass, one row past it, and chunk boundaries that fall inside a node
    "u50_63": _u50(63), "u50_64": _u50(64), "u50_65": _u50(65),
    "u50_127": _u50(127), "u50_128": _u50(128), "u50_129": _u50(129),
    # the dispatch edge between the NG = 1 and the NG = 4 tile kernel: npt 16 and 17
    "u160_560": lambda: (160,) + br.uniform(160, 560, seed=160),
    "u170_560": lambda: (170,) + br.uniform(170, 560, seed=170),
    # the smallest E at which a ws workgroup owns two / three passes of its own: the pipeline's steady state
    "u4000_32769": _multi(*gr.BN_CSR_MULTI_TILE[0]),
    "hub4000_65537": _multi(*gr.BN_CSR_MULTI_TILE[1]),
    # bf16 only: the smallest E with two / three sixteen-edge steps per stream of the chained kernel
    "u12000_98305": lambda: (12000,) + br.uniform(12000, 98305, seed=98305),
    "hub12000_196609": lambda: (12000,) + br.hub(12000, 196609, 1000, seed=196609),
})
BF16_ONLY = ("u12000_98305", "hub12000_196609")
FP32_GRAPHS = [k for k in EDGE_GRAPHS if k not in BF16_ONLY]
BF16_GRAPHS = list(EDGE_GRAPHS)

# name -> (N, E, npt, NG, tiles, ws chunk, ws grid, chain chunk)   (None: the kernel refuses the size)
EXPECT = {
    "tiny": (20, 7, 64, 4, 1, None, None, None),
    "hub65": (300, 2000, 8, 1, 38, 64, 32, 16),
    "hub150": (300, 2000, 8, 1, 38, 64, 32, 16),
    "hub1000": (300, 2000, 8, 1, 38, 64, 32, 16),
    "chain257": (257, 257, 56, 4, 5, 64, 5, 16),
    "ladder": (45, 820, 3, 1, 15, 64, 13, 16),
    "gaps": (200, 90, 64, 4, 4, 64, 2, 16),
    "u50_63": (50, 63, 44, 4, 2, None, None, 16),
    "u50_64": (50, 64, 43, 4, 2, 64, 1, 16),
    "u50_65": (50, 65, 43, 4, 2, 64, 2, 16),
    "u50_127": (50, 127, 22, 4, 3, 64, 2, 16),
    "u50_128": (50, 128, 21, 4, 3, 64, 2, 16),
    "u50_129": (50, 129, 21, 4, 3, 64, 3, 16),
    "u160_560": (160, 560, 16, 1, 10, 64, 9, 16),
    "u170_560": (170, 560, 17, 4, 10, 64, 9, 16),
    "u4000_32769": (4000, 32769, 6, 1, 667, 128, 257, 16),
    "hub4000_65537": (4000, 65537, 3, 1, 1334, 192, 342, 16),
    "u12000_98305": (12000, 98305, 6, 1, 2000, 256, 385, 32),
    "hub12000_196609": (12000, 196609, 3, 1, 4000, 448, 439, 48),
}


def csr_case(name):
    """(N, E, src, dst int64 numpy in CSR order, order, row_ptr) of an EDGE_GRAPHS entry"""
    N, src, dst = EDGE_GRAPHS[name]()
    order, row_ptr, _, _ = csr_of(src, dst, N)
    return N, len(src), src[order], dst[order], order, row_ptr


# ---------------------------------------------------------------------------------------------
# inputs: full-mantissa fp32, CPU
# ---------------------------------------------------------------------------------------------
def stage_inputs(N, E, seed, wc4_scale=0.5):
    """The operands of one fp32 case, unfolded form: dict(UV [N,128], attr [E,4] (in the order of the edge LIST, not
    CSR), wc4 [64,4], b1, s1, t1, W2 [64,64], b2, s2, t2, root [N,64]).  A quarter of s2 is negative (columns c % 4 ==
    1), t2 = -50 in the CLOSED columns (every message 0 there: the output must be the root), column ZERO_K of W2 is 0."""
    g = torch.Generator().manual_seed(seed + 100)
    s2 = torch.rand(C, generator=g) + 0.5
    s2[1::4] = -s2[1::4]
    t2 = randn32((C,), seed + 8, 0.3)
    t2[list(CLOSED)] = -50.0
    W2 = randn32((C, C), seed + 6, 1.0 / 8)
    W2[:, ZERO_K] = 0.0
    return dict(UV=randn32((N, 2 * C), seed), attr=randn32((max(E, 1), 4), seed + 1, 0.5)[:E],
                wc4=randn32((C, 4), seed + 2, wc4_scale), b1=randn32((C,), seed + 3, 0.1),
                s1=torch.rand(C, generator=g) + 0.5, t1=randn32((C,), seed + 5, 0.3), W2=W2,
                b2=randn32((C,), seed + 7, 0.1), s2=s2, t2=t2, root=randn32((N, C), seed + 9))


def fold_inputs(inp):
    """The folded form of stage_inputs, in the dtype of the operands (fp32: rounded like the product's fold, and from
    then on GIVEN operands — the reference of the folded form starts from them): UV' = s1 UV + (s1 b1 + t1 | 0),
    Wc4' = s1 Wc4, t2' = s2 b2 + t2, b1 = s1 = t1 = b2 = None (ops.fold_factorised_layer on the per-node products)"""
    s1 = inp["s1"]
    out = dict(inp)
    out["UV"] = inp["UV"] * torch.cat([s1, s1]) + torch.cat([s1 * inp["b1"] + inp["t1"], torch.zeros_like(s1)])
    out["wc4"] = inp["wc4"] * s1[:, None]
    out["t2"] = inp["s2"] * inp["b2"] + inp["t2"]
    out["b1"] = out["s1"] = out["t1"] = out["b2"] = None
    return out


def stage_inputs_bf16(N, E, seed, wc4_scale=2.0):
    """The operands of one bf16-storage case (the scales of tests/test_gpu_bf16.py): dict(UV [N,128] bf16, attr [E,4]
    fp32 (edge-LIST order), wc4 [64,4], s1 fp32, W2f [64,64] bf16 (column ZERO_K zero), t2f fp32 (CLOSED: -50), root)"""
    g = torch.Generator().manual_seed(seed + 200)
    W2f = randn32((C, C), seed + 6, 1.0 / 8)
    W2f[:, ZERO_K] = 0.0
    t2f = randn32((C,), seed + 8, 0.3)
    t2f[list(CLOSED)] = -50.0
    return dict(UV=randn32((N, 2 * C), seed).to(torch.bfloat16), attr=randn32((max(E, 1), 4), seed + 1, 0.5)[:E],
                wc4=randn32((C, 4), seed + 2, wc4_scale), s1=torch.rand(C, generator=g) + 0.5,
                W2f=W2f.to(torch.bfloat16), t2f=t2f, root=randn32((N, C), seed + 9))


# ---------------------------------------------------------------------------------------------
# float64 reference and the envelopes of the fp32 path
# ---------------------------------------------------------------------------------------------
def _node_sum(v, idx, N):
    return torch.zeros(N, v.shape[1], dtype=torch.float64, device=v.device).index_add_(0, idx, v)


def _d(t):
    return None if t is None else t.double()


def edge_stage_ref(inp, src, dst, attr, N, x6=False):
    """The stage in float64 on the operands `inp` (either form; any float dtype), CSR-ordered src / dst int64 [E] and
    attr [E,4] on the operands' device.  Returns dict(m, tol_m [E,64]: the messages and the bound of k_edge_uv_mlp2 and
    of every fused kernel's messages; out, tol [N,64]; deg [N]).

    Per message, first order, from the kernels as written (edge.hip):
      layer 1   z = u + v; four fmaf(a_i, w_i, z); z + b1; fmaf(., s1, t1): n1 = 5 (6 with b1) roundings, each relative to
                a partial sum no larger than S = |u| + |v| + |attr| . |Wc4| (+ |b1|):  d_pre = n1 u S,
                d_h1 = |s1| d_pre + u |t|   (the scale fma; ReLU is 1-Lipschitz).  Folded: d_h1 = 5 u S.
      layer 2   a 64-term dot product on the matrix core, whose order of accumulation is not ours to assume: the
                order-independent (64 + c) u sum_k |h1_k| |W2_ck|, c = 2 (C2), + layer 1's error through |W2|:
                d_acc = d_h1 . |W2|^T + (64 + c) u P,  P = h1 . |W2|^T
      epilogue  acc + b2 (u |acc + b2|, absent without b2), fmaf(., s2, t2) (u |y|):  d_y = |s2| d + u |y| = d_m.
      X6        k_edge_uv_mlp2_mean_ws<*, true> forms a . b from the exact three-way split x = h + m + l of yl_split8 (h the
                top 8 significand bits, h + m the top 16, truncated: |m| < 2^-7 |x|, |l| < 2^-15 |x|) and keeps a_h b_h,
                a_h b_m, a_m b_h, a_h b_l, a_l b_h, a_m b_m — exact bf16 products, fp32 accumulation.  It drops a_m b_l,
                a_l b_m (< 2^-22 |a b| each) and a_l b_l (< 2^-30 |a b|): X6_DROP P = (8 + 2^-6) u P more, and u |z| for
                the sum of its two accumulators.  The accumulation itself is taken at the same (64 + c) u P: the kept
                cross terms are below 2^-6 of the leading ones and the matrix core is taken to round an MFMA's sum of 16
                exact products no more than 16 separate additions would per kept k of the leading term — like dot_delta,
                an assumption about an undocumented unit, and the GPU test records how far below it the kernel stays.
                Folded, W2' = fl(s2 W2) is split (one rounding more per weight: u P) and t2 starts the accumulator
                (|t2| joins the magnitudes; no epilogue fma).
    Per output: the run sum of deg messages in CSR order, whatever the passes (a carried partial sum is continued, not
    re-rounded), the reciprocal and the product — mean_tol(sum |m|, deg) = run_sum_tol(sum |m|, deg) / deg + u sum |m| /
    deg — + sum d_m / deg, and ONE rounding of the add onto root: u |out|.  A node without in-edges: the root, bit for bit
    (tol = 0)."""
    UV = inp["UV"].double()
    b1, s1, t1, b2, s2, t2 = (_d(inp[k]) for k in ("b1", "s1", "t1", "b2", "s2", "t2"))
    a, w, w2 = attr.double(), inp["wc4"].double(), inp["W2"].double()
    fold = b1 is None and s1 is None and b2 is None
    Uu, Vv = UV[:, :C][dst], UV[:, C:2 * C][src]
    S = Uu.abs() + Vv.abs() + a.abs() @ w.abs().t()
    pre = Uu + Vv + a @ w.t()
    n1 = 5.0
    if b1 is not None:
        pre, S, n1 = pre + b1, S + b1.abs(), 6.0
    d_h1 = n1 * U * S
    t = pre
    if s1 is not None:
        t = pre * s1 + t1
        d_h1 = s1.abs() * d_h1 + U * t.abs()
    h1 = torch.relu(t)
    if x6 and fold and s2 is not None:
        w2s = w2 * s2[:, None]
        P = h1 @ w2s.abs().t() + t2.abs()
        y = h1 @ w2s.t() + t2
        d_y = d_h1 @ w2s.abs().t() + ((C + C2 + 1) * U + X6_DROP) * P + U * y.abs()
    else:
        P = h1 @ w2.abs().t()
        y = h1 @ w2.t()
        d_y = d_h1 @ w2.abs().t() + (C + C2) * U * P
        if x6:
            d_y = d_y + X6_DROP * P + U * y.abs()
        if b2 is not None:
            y = y + b2
            d_y = d_y + U * y.abs()
        if s2 is not None:
            y = y * s2 + t2
            d_y = s2.abs() * d_y + U * y.abs()
    m = torch.relu(y)
    tol_m = d_y * SLACK
    deg = torch.bincount(dst, minlength=N).double()
    d1 = deg.clamp_min(1)[:, None]
    mean = _node_sum(m, dst, N) / d1
    tol_mean = _node_sum(tol_m, dst, N) / d1 + mean_tol(_node_sum(m, dst, N), deg[:, None])     # m >= 0: sum |m| = sum m
    out = inp["root"].double() + mean
    tol = (tol_mean + U * (out.abs() + tol_mean)) * SLACK
    tol = torch.where(deg[:, None] > 0, tol, torch.zeros_like(tol))
    return dict(m=m, tol_m=tol_m, out=out, tol=tol, deg=deg)


# ---------------------------------------------------------------------------------------------
# float64 reference and the envelope of the bf16 path
# ---------------------------------------------------------------------------------------------
def midpoint_distance(v):
    """distance of v >= 0 (float64) to the nearest bf16 rounding MIDPOINT of its binade: |frac(v / ulp) - 1/2| ulp"""
    ulp = br.ulp_bf16(v)
    x = v / ulp
    return (x - torch.floor(x) - 0.5).abs() * ulp


def edge_stage_ref_bf16(inp, src, dst, attr, N, chain):
    """The bf16 stage in float64 on stage_inputs_bf16 operands: wc = s1 Wc4, z = U'[dst] + V'[src] + attr . wc^T,
    h1 = bf(relu(z)) (round to nearest even, done in float64), m = relu(h1 . W2f^T + t2f), out = root + sum m / max(deg,
    1); the kernels store bf(out).  Returns dict(out, tol, base, flip [N,64], flagged (share of the hidden activations),
    deg).

    Both kernels round h1 to bf16, use bf16 W2f and UV, accumulate in fp32 and store bf16 once.
      dz        the fp32 noise of layer 1.  k_edge_uv_mlp2_mean_h: fl(s1 Wc4), fl(u + v), four fmas: 6 u S with S = |u| +
                |v| + |attr| . |wc|.  k_edge_chain_h: at most 14 non-zero exact products enter the fp32 accumulator of
                its five MFMAs, + fl(s1 Wc4): 16 u S; and its attr term is formed from bf16 (hi, lo) pairs of attr and wc,
                w_h a_h + w_h a_l + w_l a_h: the dropped w_l a_l and the pairs' own rounding (2^-18 each) stay below
                2^-16 |attr| . |wc| (edge_chain.hip:15-19).
      flags     h1 is the SAME bf16 number in the kernel and here unless relu(z) lies within dz of a rounding midpoint
                (or within dz of 0): such an activation is flagged and may come out one spacing (taken at relu(z) + dz)
                away, + dz where the spacing is smaller than the noise.  An unflagged activation contributes nothing.
                A flagged one adds |W2f[c,k]| x that to the bound of the messages it feeds: d_flip = flip . |W2f|^T.
      layer 2   dot_delta(h1 . |W2f|^T + |t2f|, 64): exact bf16 products, fp32 accumulation, t2f added once (tile: an
                fma; chained: one more MFMA on a three-term split of t2f, exact to 2^-24).
      output    fmaf(sum, fl(1 / deg), root): (sum d_m + run_sum_tol(sum m, deg)) / deg + u sum m / deg + u |out| = delta,
                then ONE bf16 store: br.store_envelope(out, delta).
    base = store_envelope(out, delta without flips); flip = sum d_flip / deg; tol = store_envelope(out, delta + flip).
    No output may leave tol.  A node without in-edges: delta = 0, i.e. the bf16 rounding of its root row."""
    UV = inp["UV"].double()
    a = attr.double()
    wc = inp["wc4"].double() * inp["s1"].double()[:, None]
    w2, t2 = inp["W2f"].double(), inp["t2f"].double()
    Uu, Vv = UV[:, :C][dst], UV[:, C:2 * C][src]
    A = a.abs() @ wc.abs().t()
    S = Uu.abs() + Vv.abs() + A
    z = Uu + Vv + a @ wc.t()
    dz = (16.0 * U * S + 2.0 ** -16 * A) if chain else 6.0 * U * S
    v = torch.relu(z)
    flagged = ((z > 0) & (midpoint_distance(v) <= dz)) | (z.abs() <= dz)       # z < -dz: h1 = 0 on both sides
    sp = br.ulp_bf16(v + dz)
    flip = torch.where(flagged, sp + torch.where(sp < 2 * dz, dz, torch.zeros_like(dz)), torch.zeros_like(dz))
    h1 = br.bf(v)
    y = h1 @ w2.t() + t2
    d_y = br.dot_delta(h1 @ w2.abs().t() + t2.abs(), C)
    d_flip = flip @ w2.abs().t()
    m = torch.relu(y)
    deg = torch.bincount(dst, minlength=N).double()
    d1 = deg.clamp_min(1)[:, None]
    msum = _node_sum(m, dst, N)
    out = inp["root"].double() + msum / d1
    has = (deg[:, None] > 0).double()
    delta = ((_node_sum(d_y, dst, N) + run_sum_tol(msum, deg[:, None])) / d1 + U * msum / d1 + U * out.abs()) * SLACK * has
    fl = _node_sum(d_flip, dst, N) / d1
    return dict(out=out, tol=br.store_envelope(out, delta + fl), base=br.store_envelope(out, delta), flip=fl,
                flagged=float(flagged.double().mean()) if flagged.numel() else 0.0, deg=deg)


# ---------------------------------------------------------------------------------------------
# fp32 emulations (numpy, CPU)
# ---------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().float().numpy()


def split3(x):
    """yl_split8 on an fp32 numpy array: (h, m, l) fp32 with x = h + m + l exactly, h = the top 8 significand bits, h + m
    the top 16 (truncation)"""
    x = np.ascontiguousarray(x, dtype=F32)
    bits = x.view(np.uint32)
    h = (bits & np.uint32(0xffff0000)).view(F32)
    hm = (bits & np.uint32(0xffffff00)).view(F32)
    return h, hm - h, x - hm


X6_KEPT = {None: ("lh", "hl", "mh", "mm", "hm", "hh"), "hh_only": ("hh",), "no_m_terms": ("lh", "hl", "hh"),
           "no_l_terms": ("mh", "mm", "hm", "hh")}
MSG_DEFECTS_X6 = ("hh_only", "no_m_terms")


def emulate_messages(inp, src, dst, attr, x6=False, defect=None):
    """The messages [E,64] fp32 of the fp32 kernels, numpy: layer 1 statement by statement (fma32 is a correctly rounded
    fmaf), layer 2 as an fp32 matrix product (numpy's order, not the matrix core's: the envelope does not depend on it),
    the epilogue statement by statement.  x6: layer 2 from the three-way splits, per 16-wide k step the six products of
    the kernel in its order into its two accumulators — one rounding per MFMA (the 16 exact products summed in float64) —
    and their sum; folded, W2' = fl(s2 W2) is split and t2 starts the accumulator.
    defect (x6 only): "hh_only" keeps a_h b_h alone, "no_m_terms" drops every product with a middle term, "no_l_terms"
    drops only a_h b_l and a_l b_h (~2^-16 per product)."""
    UV, a, wc = _np(inp["UV"]), _np(attr), _np(inp["wc4"])
    b1, s1, t1, b2, s2, t2 = (_np(inp[k]) for k in ("b1", "s1", "t1", "b2", "s2", "t2"))
    W2 = _np(inp["W2"])
    fold = b1 is None and s1 is None and b2 is None
    z = UV[dst, :C] + UV[src, C:2 * C]
    for i in range(4):
        z = fma32(a[:, i:i + 1], wc[None, :, i], z)
    if b1 is not None:
        z = z + b1[None, :]
    if s1 is not None:
        z = fma32(z, s1[None, :], t1[None, :])
    h = np.maximum(z, F32(0))
    E = h.shape[0]
    if not x6:
        acc = h @ W2.T
    else:
        B = (W2 * s2[:, None]).astype(F32) if fold else W2
        As, Bs = dict(zip("hml", split3(h))), dict(zip("hml", split3(B)))
        accM = np.broadcast_to(t2[None, :], (E, C)).astype(F32) if fold else np.zeros((E, C), dtype=F32)
        accS = np.zeros((E, C), dtype=F32)
        kept = X6_KEPT[defect]
        for ks in range(4):
            k = slice(16 * ks, 16 * ks + 16)
            for pair in ("lh", "hl", "mh", "mm", "hm", "hh"):
                if pair not in kept:
                    continue
                p = As[pair[0]][:, k].astype(np.float64) @ Bs[pair[1]][:, k].astype(np.float64).T
                if pair in ("lh", "mh", "hm"):
                    accS = (accS.astype(np.float64) + p).astype(F32)
                else:
                    accM = (accM.astype(np.float64) + p).astype(F32)
        acc = accM + accS
        if fold:
            return np.maximum(acc, F32(0))
    if b2 is not None:
        acc = acc + b2[None, :]
    if s2 is not None:
        acc = fma32(acc, s2[None, :], t2[None, :])
    return np.maximum(acc, F32(0))


AGG_DEFECTS = ("drop_last", "boundary_twice", "carry_lost", "pass_count", "neighbour_row", "root_twice", "root_missing",
               "stale_root", "chunk_overlap")


def pass_ranges(ptr, dst, N, E, layout, overlap=False):
    """[(first row, end row, first node)] of the edge ranges the workgroups walk in passes.
    layout ("tiles", npt, pass): the CSR range of npt consecutive nodes; ("ws", chunk, pass): [w chunk, (w + 1) chunk)
    with both ends moved forward to a node boundary (edge.hip: the node holding the boundary edge starts there or the
    range starts at the next node) — a range that ends up empty is skipped.  overlap: the start is NOT moved."""
    kind, par = layout[0], layout[1]
    out = []
    if kind == "tiles":
        for n0 in range(0, N, par):
            out.append((int(ptr[n0]), int(ptr[min(N, n0 + par)]), n0))
        return out

    def bound(c):
        if c <= 0:
            return 0
        if c >= E:
            return E
        n = int(dst[c])
        return c if int(ptr[n]) == c else int(ptr[n + 1])
    for c_lo in range(0, E, par):
        eS, eE = (c_lo if overlap else bound(c_lo)), bound(c_lo + par)
        if eS < eE:
            out.append((eS, eE, int(dst[eS])))
    return out


def emulate_aggregate(msg, ptr, root, N, layout, defect=None, fused=False):
    """out [N,64] fp32: f_out pre-loaded with `root`, then per workgroup range and per pass the rows of every node of the
    pass added in ascending order to its running sum (started at 0, or at the sum carried from the pass before, with its
    count); a node that ends in the pass gets mul_rn(sum, fl(1 / cnt)) + f_out row (fused: fmaf(sum, inv, row), the bf16
    kernels).  Without a defect the result does not depend on the layout.
    defect: "drop_last" the last row of a run is not added; "boundary_twice" the first row of a pass that continues a node
    is added twice; "carry_lost" the carried sum is dropped from the third pass of a node on; "pass_count" the divisor is
    the node's row count in its LAST pass; "neighbour_row" every run starts one row late, its first row goes to the node
    in front; "root_twice" / "root_missing"; "stale_root" the SECOND node an aggregation thread finishes (ws: the k-th node
    of the pass, k >= 16; tiles: node n0 + j, j >= 16) is added to the f_out row of its first; "chunk_overlap" a ws range
    starts at its chunk boundary even inside a node, whose tail is then averaged and added a second time."""
    f = F32
    msg = np.asarray(msg, dtype=f)
    E = msg.shape[0]
    ptr = np.asarray(ptr, dtype=np.int64)
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
    if defect == "neighbour_row" and E:
        dst = dst.copy()
        starts = ptr[:-1][(np.diff(ptr) > 0) & (ptr[:-1] > 0)]
        dst[starts] = dst[starts - 1]
    root = np.asarray(root, dtype=f)
    out = root.copy()
    plen = layout[2]
    with np.errstate(all="ignore"):
        for eS, eE, n_first in pass_ranges(ptr, dst, N, E, layout, overlap=defect == "chunk_overlap"):
            carry, ccnt, cpass = None, 0, 0
            for c0 in range(eS, eE, plen):
                c1 = min(c0 + plen, eE)
                d = dst[c0:c1]
                cut = np.flatnonzero(np.diff(d)) + 1
                los = np.concatenate([[0], cut]) + c0
                his = np.concatenate([cut, [c1 - c0]]) + c0
                nseg = len(los)
                for k in range(nseg):
                    lo, hi, node = int(los[k]), int(his[k]), int(dst[los[k]])
                    cont_in = k == 0 and c0 > eS and dst[c0 - 1] == node
                    cont_out = k == nseg - 1 and c1 < eE and dst[c1] == node
                    sm, cn, npass = np.zeros(C, dtype=f), 0, 0
                    if cont_in:
                        sm, cn, npass = carry, ccnt, cpass
                        if defect == "carry_lost" and npass >= 2:
                            sm = np.zeros(C, dtype=f)
                        if defect == "boundary_twice":
                            sm = sm + msg[lo]
                    last = hi - 1 if (defect == "drop_last" and not cont_out) else hi
                    for r in range(lo, last):
                        sm = sm + msg[r]
                    cn += hi - lo
                    if cont_out:
                        carry, ccnt, cpass = sm, cn, npass + 1
                        continue
                    inv = f(1) / f(hi - lo if defect == "pass_count" else cn)
                    row = out[node]
                    j = k if layout[0] == "ws" else node - n_first
                    if defect == "stale_root" and j >= 16:
                        row = root[int(dst[los[k - 16]])] if layout[0] == "ws" else root[node - 16]
                    if defect == "root_missing":
                        row = np.zeros(C, dtype=f)
                    if defect == "root_twice":
                        row = row + root[node]
                    out[node] = fma32(sm, inv, row) if fused else (sm * inv).astype(f) + row
    return out


def emulate_stage(inp, src, dst, attr, ptr, N, layout, x6=False, defect=None):
    """emulate_messages + emulate_aggregate: f_out [N,64] fp32 of one fp32 kernel form"""
    md = defect if defect in X6_KEPT else None
    ad = defect if defect in AGG_DEFECTS else None
    return emulate_aggregate(emulate_messages(inp, src, dst, attr, x6, md), ptr, _np(inp["root"]), N, layout, ad)


BF16_DEFECTS = ("h1_truncated", "deg0_unwritten")


def emulate_stage_bf16(inp, src, dst, attr, ptr, N, layout, chain=False, defect=None):
    """The bf16 kernels in fp32 on the CPU, returned as a bfloat16 torch tensor [N,64].  Node tiles: wc = fl(s1 Wc4),
    z = fl(u + v), four fmas, ReLU, round to nearest even to bf16; chained: the attr term from the bf16 (hi, lo) pairs,
    w_h a_h + w_h a_l + w_l a_h, added to u + v with one rounding (exact products into an fp32 accumulator).  Layer 2: fp32
    product of the bf16 values, + t2f, ReLU; the run sums of emulate_aggregate; fmaf(sum, fl(1 / deg), root); one bf16
    store.  A node without in-edges: the root row, rounded.
    defect: any of AGG_DEFECTS; "h1_truncated": h1 stored by truncation; "deg0_unwritten": a node without in-edges keeps
    the buffer's fill (NaN)."""
    UV = inp["UV"].float().numpy()
    a = _np(attr)
    wc = (_np(inp["wc4"]) * _np(inp["s1"])[:, None]).astype(F32)
    u, v = UV[dst, :C], UV[src, C:2 * C]
    if chain:
        def pair(x):
            hi = torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()
            lo = torch.from_numpy(np.ascontiguousarray(x - hi)).to(torch.bfloat16).float().numpy()
            return hi.astype(np.float64), lo.astype(np.float64)
        (wh, wl), (ah, al) = pair(wc), pair(a)
        z = (u.astype(np.float64) + v.astype(np.float64) + ah @ wh.T + al @ wh.T + ah @ wl.T).astype(F32)
    else:
        z = u + v
        for i in range(4):
            z = fma32(a[:, i:i + 1], wc[None, :, i], z)
    h = torch.from_numpy(np.maximum(z, F32(0)))
    h = (br.truncate_bf16(h) if defect == "h1_truncated" else h.to(torch.bfloat16)).float().numpy()
    acc = h @ inp["W2f"].float().numpy().T
    m = np.maximum(acc + _np(inp["t2f"])[None, :], F32(0))
    ad = defect if defect in AGG_DEFECTS else None
    out = torch.from_numpy(emulate_aggregate(m, ptr, _np(inp["root"]), N, layout, ad, fused=True)).to(torch.bfloat16)
    if defect == "deg0_unwritten":
        out[torch.from_numpy(np.diff(np.asarray(ptr)) == 0)] = float("nan")
    return out
