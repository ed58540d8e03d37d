"""GPU tests (-m gpu) of the fp32 graph ops of the training step — the mean aggregation and its backward, the scatter and
per-node sums behind the first edge Linear, the factorised first edge Linear, BnCsrGrad in its two- and one-kernel
forms, the segment pooling (csrc/edge_ops.hip, bn_csr.hip, segment.hip) — per element against float64 references with
derived bounds (tests/graph_ref.py; tests/test_graph_ref_host.py shows on the CPU that every bound accepts an fp32
emulation of the kernel and rejects a dropped or doubled row, a wrong divisor and sums lost between tiles).

Graphs: the hub graphs, the 7-edge graph and the chain of test_gpu_bf16_storage_ops.py, and the ladder (in-degree n at
node n = 0..40: every tail length behind 0..5 full trips of the unrolled row loops).  BnCsrGrad also runs at E = 32769
and 65537, the smallest sizes at which a workgroup of the one-kernel backward owns two and three tiles.

Conventions (those of test_gpu_bf16_storage_ops.py): operands live in column slots of wider buffers pre-filled with
NaN; after the call everything outside the output slots must hold the bits it held before; each op runs twice and must
return the same bits.  Inputs are full-mantissa fp32 values from seeded CPU generators; the float64 references are
evaluated on the device.  Nothing is compared at a tensor's maximum; each check prints its worst error / tolerance."""
import functools

import numpy as np
import pytest
import torch

import graph_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
U = gr.U
NAN = float("nan")


def _ops():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv.ops


def _lib():
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    return lib, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Buf(object):
    """[rows + 3, sum of the slot widths (each padded to 8 columns) + 8] NaN-filled fp32 buffer; slot(i) = rows x width
    view; slots(i, j) = the view over the adjacent slots i..j (their widths multiples of 8)"""

    def __init__(self, rows, widths):
        self.rows, self.cols, c = rows, [], 0
        for w in widths:
            self.cols.append((c, c + w))
            c += -(-w // 8) * 8
        self.buf = torch.full((rows + 3, c + 8), NAN, dtype=F32, device=DEV)
        self.snap = None

    def slot(self, i):
        lo, hi = self.cols[i]
        return self.buf[:self.rows, lo:hi]

    def slots(self, i, j):
        return self.buf[:self.rows, self.cols[i][0]:self.cols[j][1]]

    def snapshot(self):
        self.snap = self.buf.clone()

    def untouched_outside(self, outs):
        """every element outside the output slots `outs` holds the bits of the snapshot (padding: still NaN)"""
        mask = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        for i in outs:
            lo, hi = self.cols[i]
            mask[:self.rows, lo:hi] = False
        pad = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        for lo, hi in self.cols:
            pad[:self.rows, lo:hi] = False
        return torch.equal(_bits(self.buf)[mask], _bits(self.snap)[mask]) and bool(torch.isnan(self.buf[pad]).all())


def _strided(t, ld):
    """the values of t [M,C] as a view with row stride `ld` floats of a NaN-filled buffer (an UNALIGNED row layout)"""
    b = torch.full((t.shape[0] + 3, ld), NAN, dtype=F32, device=DEV)
    v = b[:t.shape[0], :t.shape[1]]
    v.copy_(t)
    return v


def _vec(n, fill=NAN):
    """([n] view, [n + 8] buffer) fp32: the tail must stay NaN"""
    b = torch.full((n + 8,), NAN, dtype=F32, device=DEV)
    b[:n] = fill
    return b[:n], b


def _tail_is_nan(b, n):
    return bool(torch.isnan(b[n:]).all())


def _worst(op, name, got, want, tol):
    """asserts |got - want| <= tol (elementwise, NaN fails); prints and returns the worst error / tolerance"""
    err = (got.double() - want).abs()
    ok = err <= tol
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("ratio %-18s %-12s %.3f" % (op, name, ratio))
    assert bool(ok.all()), "%s %s: %d of %d outside the tolerance, worst error / tolerance %.3f" % (
        op, name, int((~ok).sum()), ok.numel(), ratio)
    return ratio


def _graph(N, src, dst, seed=0):
    """(ops.Graph, CSR-ordered src / dst int64 device tensors, CSR-ordered attr) — the CSR order is derived with numpy
    (stable sort by destination) and the prepared graph is checked against it"""
    ops = _ops()
    E = len(src)
    attr = np.random.default_rng(seed + E).standard_normal((E, 4)).astype(np.float32) * 0.5
    g = ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).to(DEV), torch.from_numpy(attr).to(DEV), None, N, 1)
    g.check_status()
    order, row_ptr, col_ptr, _ = gr.csr_of(src, dst, N)
    s, d, a = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (src[order], dst[order], attr[order]))
    assert torch.equal(g.src[:E].long(), s) and torch.equal(g.dst[:E].long(), d) and torch.equal(g.attr[:E], a)
    assert torch.equal(g.row_ptr.long().cpu(), torch.from_numpy(row_ptr))
    g.ensure_csc()
    assert torch.equal(g.col_ptr.long().cpu(), torch.from_numpy(col_ptr))
    return g, s, d, a


@functools.lru_cache(maxsize=None)
def _named_graph(name):
    N, src, dst = gr.GRAPHS[name]()
    return (N, len(src)) + _graph(N, src, dst)


def _twice(run):
    """run() -> tuple of tensors, called twice: the same bits; returns the first result"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    return a


# ---------------------------------------------------------------------------------------------
# mean aggregation
# ---------------------------------------------------------------------------------------------
def _mean_fwd_case(graph, mode, C):
    N, E, g, s, d, _ = _named_graph(graph)
    seed = N + E + C
    pro, acc = mode.startswith("pro"), mode.endswith("acc")
    bh = Buf(E, [C])
    bh.slot(0).copy_(gr.randn32((E, C), seed).to(DEV))
    bh.snapshot()
    h_pro = tuple(t.to(DEV) for t in gr.pro_scale_shift(C, seed + 1)) if pro else None
    base = gr.randn32((N, C), seed + 2, 1.0, 3.0).to(DEV)
    return N, E, g, d, bh, h_pro, base, pro, acc


def _mean_fwd_run(H, g, bo, base, h_pro, pro, acc):
    ops = _ops()
    out = bo.slot(0)

    def run():
        out.copy_(base if acc else torch.full_like(base, NAN))
        bo.snapshot()
        ops.csr_mean_fwd(H, g, out, h_pro=h_pro, h_relu=pro, accumulate=acc)
        assert bo.untouched_outside([0])
        return (out.clone(),)
    return _twice(run)[0]


@pytest.mark.parametrize("mode", ["plain", "pro", "acc", "pro_acc"])
@pytest.mark.parametrize("C", [64, 128, 20])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_csr_mean_fwd_fp32_matches_fp64(graph, C, mode):
    """ops.csr_mean_fwd on fp32 H: out (+)= mean over the CSR row of relu(H scale + shift).  C = 64 runs k_csr_mean_fwd_v4
    (16 lanes per node, eight rows in flight, a clamped 1..7-row tail), C = 128 and 20 the scalar k_csr_mean_fwd.
    Tolerance per node and column (graph_ref.csr_mean_fwd_ref): (deg + 3) u sum |pro(h)| / deg for the additions, the
    rounded reciprocal and the product, + u sum |t| / deg for the prologue's fma, + u (|base| + |mean|) accumulating.
    A node without in-edge: the base bit for bit when accumulating, else exactly 0."""
    N, E, g, d, bh, h_pro, base, pro, acc = _mean_fwd_case(graph, mode, C)
    got = _mean_fwd_run(bh.slot(0), g, Buf(N, [C]), base, h_pro, pro, acc)
    assert bh.untouched_outside([])
    sc, sh = h_pro if pro else (None, None)
    want, tol, deg = gr.csr_mean_fwd_ref(bh.slot(0), sc, sh, pro, d, N, base if acc else None)
    _worst("csr_mean_fwd C=%d" % C, "out", got, want, tol)
    empty = deg == 0
    assert bool(empty.any()) or graph == "chain257"
    if acc:
        assert torch.equal(_bits(got[empty]), _bits(base[empty]))
    else:
        assert bool((got[empty] == 0).all())


@pytest.mark.parametrize("mode", ["plain", "pro_acc"])
def test_csr_mean_fwd_vector_kernel_returns_the_bits_of_the_scalar_kernel(mode):
    """edge_ops.hip says of k_csr_mean_fwd_v4: "results are bit-identical to the scalar kernel".  The same C = 64 values
    through a row stride of 66 floats (no 16-byte rows) select the scalar kernel: the same bits, on the ladder."""
    N, E, g, d, bh, h_pro, base, pro, acc = _mean_fwd_case("ladder", mode, 64)
    vec = _mean_fwd_run(bh.slot(0), g, Buf(N, [64]), base, h_pro, pro, acc)
    hs = _strided(bh.slot(0), 66)
    assert hs.stride(0) == 66 and torch.equal(_bits(hs), _bits(bh.slot(0)))
    sca = _mean_fwd_run(hs, g, Buf(N, [64]), base, h_pro, pro, acc)
    assert torch.equal(_bits(vec), _bits(sca))


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_csr_mean_bwd_fp32_is_the_rounded_product_with_the_reciprocal(graph, C):
    """ops.csr_mean_bwd to fp32 (C = 64: k_csr_mean_bwd_v4, C = 128: the scalar k_csr_mean_bwd): dM[q] = d_out[dst_q] *
    fl(1 / max(deg, 1)) — BIT equal to that fp32 arithmetic done by torch (IEEE division and product), and within
    2 u |q| of the float64 quotient q = d_out / deg (the reciprocal's rounding and the product's)."""
    ops = _ops()
    N, E, g, s, d, _ = _named_graph(graph)
    bo = Buf(N, [C])
    bo.slot(0).copy_(gr.randn32((N, C), N + E + C + 9).to(DEV))
    bo.snapshot()
    bm = Buf(E, [C])
    bm.snapshot()
    dM = bm.slot(0)

    def run():
        dM.fill_(NAN)
        ops.csr_mean_bwd(bo.slot(0), g, dM)
        return (dM.clone(),)
    got = _twice(run)[0]
    assert bm.untouched_outside([0]) and bo.untouched_outside([])
    assert torch.equal(_bits(got), _bits(gr.csr_mean_bwd_fp32(bo.slot(0), d, N)))
    q = gr.csr_mean_bwd_ref(bo.slot(0), d, N)
    _worst("csr_mean_bwd C=%d" % C, "dM", got, q, 2.0 * U * q.abs())


# ---------------------------------------------------------------------------------------------
# backward of the two gathers, per-node sums of the factorised backward
# ---------------------------------------------------------------------------------------------
def _scatter_run(dG, Cin, g, N, base, acc):
    ops = _ops()
    bx = Buf(N, [Cin])
    dX = bx.slot(0)

    def run():
        dX.copy_(base if acc else torch.full_like(base, NAN))
        bx.snapshot()
        ops.edge_scatter_bwd(dG, Cin, g, dX, accumulate=acc)
        assert bx.untouched_outside([0])
        return (dX.clone(),)
    return _twice(run)[0]


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("Cin", [64, 5])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_edge_scatter_bwd_matches_fp64(graph, Cin, acc):
    """ops.edge_scatter_bwd: dX[n] (+)= sum over the CSR row of dG[:, :Cin] + sum over the CSC column of dG[:, Cin:] —
    Cin = 64: k_edge_scatter_bwd_v4 (four clamped row loads per trip), Cin = 5: the scalar kernel.  One accumulator over
    both runs: (deg_in + deg_out + 2) u sum |terms|, + u (|base| + |sum|) accumulating.  A node without any edge: the
    base bit for bit, else exactly 0."""
    N, E, g, s, d, _ = _named_graph(graph)
    seed = N + E + Cin
    bg = Buf(E, [2 * Cin])
    bg.slot(0).copy_(gr.randn32((E, 2 * Cin), seed).to(DEV))
    bg.snapshot()
    base = gr.randn32((N, Cin), seed + 1, 1.0, 3.0).to(DEV)
    got = _scatter_run(bg.slot(0), Cin, g, N, base, acc)
    assert bg.untouched_outside([])
    want, tol = gr.edge_scatter_bwd_ref(bg.slot(0), Cin, s, d, N, base if acc else None)
    _worst("edge_scatter_bwd Cin=%d" % Cin, "dX", got, want, tol)
    lone = (torch.bincount(d, minlength=N) + torch.bincount(s, minlength=N)) == 0
    assert bool(lone.any()) or graph == "chain257"
    if acc:
        assert torch.equal(_bits(got[lone]), _bits(base[lone]))
    else:
        assert bool((got[lone] == 0).all())


@pytest.mark.parametrize("acc", [False, True])
def test_edge_scatter_bwd_vector_kernel_returns_the_bits_of_the_scalar_kernel(acc):
    """k_edge_scatter_bwd_v4: "same summation order as the scalar kernel" — the same Cin = 64 values through a row stride
    of 130 floats select the scalar kernel: the same bits, on the ladder."""
    N, E, g, s, d, _ = _named_graph("ladder")
    bg = Buf(E, [128])
    bg.slot(0).copy_(gr.randn32((E, 128), 77).to(DEV))
    base = gr.randn32((N, 64), 78, 1.0, 3.0).to(DEV)
    vec = _scatter_run(bg.slot(0), 64, g, N, base, acc)
    gs = _strided(bg.slot(0), 130)
    assert gs.stride(0) == 130
    assert torch.equal(_bits(vec), _bits(_scatter_run(gs, 64, g, N, base, acc)))


@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_edge_uv_sums_match_fp64(graph):
    """yolat_edge_uv_sums (both halves of dUV: dU over the CSR row, eight rows in flight and a clamped tail; dV over the
    CSC column, gathered by slot, eight clamped loads per trip) and yolat_edge_uv_sums_v with half = 0 (the dV half alone:
    columns [0, 64) keep their bits) against per-node float64 sums within (deg + 2) u sum |terms|; the dV halves of the
    two entry points are the same bits."""
    lib, check = _lib()
    N, E, g, s, d, _ = _named_graph(graph)
    bh = Buf(E, [64])
    bh.slot(0).copy_(gr.randn32((E, 64), N + E + 21).to(DEV))
    bh.snapshot()
    dH = bh.slot(0)
    buv = Buf(N, [64, 64])
    dUV = buv.slots(0, 1)
    assert dUV.shape == (N, 128)
    keep = gr.randn32((N, 64), N + E + 22).to(DEV)

    def run_both():
        dUV.fill_(NAN)
        buv.snapshot()
        check(lib.yolat_edge_uv_sums(dH.data_ptr(), dH.stride(0), g.row_ptr.data_ptr(), g.col_ptr.data_ptr(),
                                     g.slots.data_ptr(), N, 64, dUV.data_ptr(), dUV.stride(0), _stream()), "yolat_edge_uv_sums")
        assert buv.untouched_outside([0, 1])
        return (dUV.clone(),)

    def run_v():
        dUV.fill_(NAN)
        buv.slot(0).copy_(keep)
        buv.snapshot()
        check(lib.yolat_edge_uv_sums_v(dH.data_ptr(), dH.stride(0), 0, g.col_ptr.data_ptr(), g.slots.data_ptr(), N, 64,
                                       dUV.data_ptr(), dUV.stride(0), _stream()), "yolat_edge_uv_sums_v")
        assert buv.untouched_outside([1])                              # columns [0, 64): the bits of `keep`
        return (dUV.clone(),)
    both, only_v = _twice(run_both)[0], _twice(run_v)[0]
    assert bh.untouched_outside([])
    wu, tu, wv, tv = gr.edge_uv_sums_ref(dH, s, d, N)
    _worst("edge_uv_sums", "dU", both[:, :64], wu, tu)
    _worst("edge_uv_sums", "dV", both[:, 64:], wv, tv)
    _worst("edge_uv_sums_v", "dV", only_v[:, 64:], wv, tv)
    assert torch.equal(_bits(only_v[:, :64]), _bits(keep)) and torch.equal(_bits(only_v[:, 64:]), _bits(both[:, 64:]))


# ---------------------------------------------------------------------------------------------
# factorised first edge Linear
# ---------------------------------------------------------------------------------------------
def _check_stats(op, st, M, N, v, dv):
    """st: the flat fp32 statistics buffer (NaN-filled before the call); v / dv: float64 values and their bound"""
    G = (M + 31) // 32
    n = 2 * G * N
    got = st[:n].view(G, N, 2)
    s, m2, ts, tm = gr.group_stats_ref(v, dv)
    _worst(op, "stats sum", got[:, :, 0], s, ts)
    _worst(op, "stats M2", got[:, :, 1], m2, tm)
    assert _tail_is_nan(st, n), "%s: statistics written past the last row group" % op


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("with_b1", [False, True])
@pytest.mark.parametrize("E,kind", gr.EDGE_CASES)
def test_edge_uv_lin1_fwd_fp32_matches_fp64(E, kind, with_b1, with_stats):
    """yolat_edge_uv_lin1_fwd through the library with a GIVEN fp32 UV: H1[q] = U[dst_q] + V[src_q] + Wc4 . attr_q + b1,
    six roundings (u + v, four fmas, + b1) relative to partial sums no larger than S = |u| + |v| + |attr| . |Wc4| + |b1|:
    6 u S.  Statistics (sum, M2 about the group mean) per 32-row group, the last group short, nothing written past it:
    bf16_ref.group_stats_ref from the same bound.  The row counts are the bf16 twin's."""
    ops = _ops()
    lib, check = _lib()
    N, src, dst = gr.edge_case_graph(E, kind)
    g, s, d, attr = _graph(N, src, dst)
    seed = 3 * E + N
    buv = Buf(N, [128])
    buv.slot(0).copy_(gr.randn32((N, 128), seed).to(DEV))
    buv.snapshot()
    wc4 = gr.randn32((64, 4), seed + 1, 0.5).to(DEV)
    b1 = gr.randn32((64,), seed + 2, 0.3).to(DEV) if with_b1 else None
    bh = Buf(E, [64])
    bh.snapshot()
    H1, UV = bh.slot(0), buv.slot(0)
    stats = []

    def run():
        H1.fill_(NAN)
        st = None
        if with_stats:
            st = ops.stats_buffer(E, 64, DEV)
            st.fill_(NAN)
        check(lib.yolat_edge_uv_lin1_fwd(UV.data_ptr(), UV.stride(0), g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                         E, wc4.data_ptr(), b1.data_ptr() if with_b1 else None, 64, H1.data_ptr(),
                                         H1.stride(0), st.data_ptr() if with_stats else None, _stream()),
              "yolat_edge_uv_lin1_fwd")
        stats.append(st)
        return (H1.clone(),)
    got = _twice(run)[0]
    assert bh.untouched_outside([0]) and buv.untouched_outside([])
    want, delta = gr.edge_uv_lin1_ref(UV, s, d, attr, wc4, b1)
    _worst("edge_uv_lin1_fwd", "H1", got, want, delta)
    if with_stats:
        assert torch.equal(_bits(stats[0]), _bits(stats[1]))
        _check_stats("edge_uv_lin1_fwd", stats[0], E, 64, want, delta)


# ---------------------------------------------------------------------------------------------
# BatchNorm + ReLU + mean aggregation backward, never materialised
# ---------------------------------------------------------------------------------------------
_BN = {}


def _bn_csr_case(N, E, kind):
    """the device operands of one case and the float64 reference of its statistics: built once, shared by the three
    forms, never written (the buffers' snapshots are checked after every form)"""
    key = (N, E, kind)
    if key not in _BN:
        _BN.clear()                                                     # one case at a time
        src, dst = gr.bn_csr_graph(N, E, kind)
        g, s, d, _ = _graph(N, src, dst)
        inp = {k: v.to(DEV) for k, v in gr.bn_csr_inputs(N, E, 5 * N + E).items()}
        b = Buf(E, [64, 64, 64])                                        # Y | A | dA
        b.slot(0).copy_(inp["Y"])
        b.slot(1).copy_(inp["A"])
        b.snapshot()
        bo = Buf(N, [64])
        bo.slot(0).copy_(inp["d_out"])
        bo.snapshot()
        coefs = (inp["mean"], inp["invstd"], inp["scale"], inp["shift"])
        stats_ref = gr.bn_csr_stats_ref(bo.slot(0), d, N, b.slot(0), *coefs)
        assert float((~stats_ref[0]["sure"]).double().mean()) <= gr.KINK_SHARE
        _BN[key] = (g, d, inp, b, bo, coefs, stats_ref)
    return _BN[key]


BN_FORMS = ["two_kernel", "one_kernel", "one_kernel_next"]


@pytest.mark.parametrize("form", BN_FORMS)
@pytest.mark.parametrize("N,E,kind", gr.BN_CSR_CASES)
def test_bn_csr_grad_fp32_matches_fp64(N, E, kind, form):
    """ops.BnCsrGrad on fp32 Y (bn_csr.hip): stats(), then the consumers of the never-materialised dY —
      two_kernel        bwd_w() (yolat_linear_bwd_w_csr: dW, db) and fwd_wt() (yolat_linear_fwd_wt_csr: dA): fp32 only
      one_kernel        bwd_w_and_x() (k_bn_csr_l2_bwd<float>: dW, db and dA from one pass over the tiles)
      one_kernel_next   the same with the next BatchNorm's backward statistics
    The cases are those of the bf16 twin and (4000, 32769, uniform): 513 tiles, two per workgroup, the last workgroup one;
    (4000, 65537, hub1000): 1025 tiles, three per workgroup, the last two — the smallest E at which the prefetch chain
    fetch(tile + 1) / fetch_idx(tile + 2) and the cross-tile accumulators accw, dbacc, p1, p2 run.

    Reference: the float64 backward of mean-aggregate(relu(batchnorm(Y))) (graph_ref; checked against autograd in
    test_graph_ref_host.py).  Tolerances, per output (u = 2^-24; no bfloat16 terms in this precision):
      dgamma, dbeta, (c1, c2) = sums / E:  (min(E, 640) + 8) u sum |terms| + the full magnitude of the terms within 1e-4 of
          the ReLU kink (at most 0.1 % of the elements)
      dY (never stored; formed from the kernel's OWN fp32 (c1, c2)):  d_dY = 10 u |scale| (|g| + |c1| + |xhat c2|), + |scale g|
          on the kink
      dW = dY^T . A1:   d_dY^T . |A1| + 2 (E + 2) u |dY|^T . |A1|  (+ |dY|^T . u |t|: A1 = relu(fma(A, a_scale, a_shift)) of
          full-mantissa A rounds once)
      db = sum dY:      sum d_dY + (E + 2) u sum |dY|
      dA = dY . W:      d_dY . |W| + dot_delta(|dY| . |W|, 64)
      next BatchNorm:   float64 sums of the kernel's STORED dA:  (64 ceil(tiles / 512) + 6) u sum |terms|, no kink term: the
          kernel's mask fmaf(A, a_scale, a_shift) > 0 is the float64 one (graph_ref.relu_mask_is_exact, host test)."""
    ops = _ops()
    g, d, inp, b, bo, (mean, invstd, scale, shift), (ref, g0, tol_b, tol_g) = _bn_csr_case(N, E, kind)
    Y, A, dA = b.slot(0), b.slot(1), b.slot(2)
    a_pro, W, m1, is1 = (inp["a_scale"], inp["a_shift"]), inp["W"], inp["m1"], inp["is1"]
    with_next = form == "one_kernel_next"

    def run():
        dA.fill_(NAN)
        dg, dg_buf = _vec(64)
        dbt, dbt_buf = _vec(64)
        dbias, dbias_buf = _vec(64)
        ng, ng_buf = _vec(64)
        nb, nb_buf = _vec(64)
        bw = Buf(64, [64])
        bw.snapshot()
        h = ops.BnCsrGrad(bo.slot(0), g, Y, mean, invstd, scale, shift, relu=True)
        h.stats(dg, dbt)
        coef = h.coef.clone()
        coef1 = None
        if form == "two_kernel":
            h.bwd_w(A, bw.slot(0), dbias, a_pro=a_pro, a_relu=True)
            h.fwd_wt(W, dA)
        else:
            coef1 = h.bwd_w_and_x(A, W, bw.slot(0), dbias, dA, a_pro=a_pro, a_relu=True,
                                  next_bn=(m1, is1, ng, nb) if with_next else None)
        assert bw.untouched_outside([0])
        for buf in (dg_buf, dbt_buf, dbias_buf, ng_buf, nb_buf):
            assert _tail_is_nan(buf, 64)
        out = [dg.clone(), dbt.clone(), coef, bw.slot(0).clone(), dbias.clone(), dA.clone()]
        if with_next:
            out += [ng.clone(), nb.clone(), coef1.clone()]
        else:
            assert coef1 is None and bool(torch.isnan(ng).all()) and bool(torch.isnan(nb).all())
        return out
    got = _twice(run)
    assert b.untouched_outside([2]) and bo.untouched_outside([])
    dg, dbt, coef, dW, dbias, dA_got = got[:6]
    op = "bn_csr " + form
    _worst(op, "dgamma", dg, ref["dgamma"], tol_g)
    _worst(op, "dbeta", dbt, ref["dbeta"], tol_b)
    _worst(op, "c1", coef[:64], ref["c1"], tol_b / E)
    _worst(op, "c2", coef[64:], ref["c2"], tol_g / E)
    dY, d_dY = gr.bn_csr_dy_ref(g0, Y, mean, invstd, scale, shift, coef)
    con = gr.bn_csr_consumers_ref(dY, d_dY, A, a_pro[0], a_pro[1], True, W)
    _worst(op, "dW", dW, con["dW"], con["tol_dW"])
    _worst(op, "db", dbias, con["db"], con["tol_db"])
    _worst(op, "dA", dA_got, con["dA"], con["tol_dA"])
    if with_next:
        ng, nb, coef1 = got[6:]
        want_b, t1, want_g, t2 = gr.next_bn_ref(dA_got, A, a_pro[0], a_pro[1], m1, is1)
        _worst(op, "next dbeta", nb, want_b, t1)
        _worst(op, "next dgamma", ng, want_g, t2)
        _worst(op, "next c1", coef1[:64], want_b / E, t1 / E)
        _worst(op, "next c2", coef1[64:], want_g / E, t2 / E)


# ---------------------------------------------------------------------------------------------
# segment pooling
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segments():
    """(graph, sizes, bbox_idx int64 device, ptr numpy, N, P, rows of the planted segments) on segment_ladder()"""
    ops = _ops()
    sizes = gr.segment_ladder()
    bb, ptr = gr.segment_ids(sizes)
    N, P = len(bb), len(sizes)
    bbd = torch.from_numpy(bb).to(DEV)
    g = ops.build_graph(torch.zeros(0, 2, dtype=torch.int64, device=DEV), torch.zeros(0, 4, device=DEV), bbd, N, P)
    g.check_status()
    assert torch.equal(g.seg_ptr.long().cpu(), torch.from_numpy(ptr))
    assert torch.equal(g.node_seg[:N].long(), bbd)
    plant = dict(tie78=int(ptr[int(np.argmax(sizes))]),                  # the 300-row segment: rows 7 and 8 equal
                 tie09=int(ptr[int(np.nonzero(sizes == 40)[0][0])]),     # the 40-row segment: rows 0 and 9 equal
                 negative=(int(ptr[int(np.nonzero(sizes == 17)[0][0])]), 17))
    return g, sizes, bbd, ptr, N, P, plant


def _segment_x(D):
    """X [N,D] fp32 on the CPU with the planted rows: two ties of the maximum across the eight-row trip boundary, and one
    segment whose prologue'd values are all negative (scale >= 0.5, |shift| small: -100 stays negative)"""
    g, sizes, bbd, ptr, N, P, plant = _segments()
    X = gr.randn32((N, D), 100 + D)
    top = gr.randn32((2, D), 101 + D, 1.0, 50.0)
    X[plant["tie78"] + 7] = X[plant["tie78"] + 8] = top[0]
    X[plant["tie09"]] = X[plant["tie09"] + 9] = top[1]
    r0, n = plant["negative"]
    X[r0:r0 + n] = -100.0 + gr.randn32((n, D), 102 + D)
    return X


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("D", gr.SEGMENT_D)
def test_segment_mean_fwd_matches_fp64(D, pro):
    """ops.segment_mean_fwd on segment_ladder() (sizes 0..40 and 300: every tail behind 0..5 eight-row trips, and 37 trips
    with a 4-row tail), with and without the (scale, shift) + ReLU prologue.  k_segment_mean_fwd adds the rows in order
    and DIVIDES by the count: (cnt + 2) u sum |terms| / cnt, + u sum |t| / cnt for the prologue's fma.  An empty segment: 0."""
    ops = _ops()
    g, sizes, bbd, ptr, N, P, plant = _segments()
    bx = Buf(N, [D])
    bx.slot(0).copy_(_segment_x(D).to(DEV))
    bx.snapshot()
    x_pro = tuple(t.to(DEV) for t in gr.pro_scale_shift(D, 103 + D)) if pro else None
    by = Buf(P, [D])
    by.snapshot()
    Y = by.slot(0)

    def run():
        Y.fill_(NAN)
        ops.segment_mean_fwd(bx.slot(0), g, Y, x_pro=x_pro, x_relu=pro)
        return (Y.clone(),)
    got = _twice(run)[0]
    assert by.untouched_outside([0]) and bx.untouched_outside([])
    sc, sh = x_pro if pro else (None, None)
    want, tol, cnt = gr.csr_mean_fwd_ref(bx.slot(0), sc, sh, pro, bbd, P, divides=True)
    _worst("segment_mean_fwd D=%d" % D, "Y", got, want, tol)
    assert bool((cnt == 0).any()) and bool((got[cnt == 0] == 0).all())


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("D", gr.SEGMENT_D)
def test_segment_max_fwd_is_the_first_argmax_bit_for_bit(D, pro):
    """ops.segment_max_fwd: value and arg EQUAL a first-occurrence argmax (graph_ref.first_argmax) of the fp32 values —
    with the prologue those of the correctly rounded fmaf (graph_ref.fma32) and ReLU.  Planted: rows 7 and 8 of the
    300-row segment and rows 0 and 9 of the 40-row segment hold the maximum of every column twice, on either side of the
    eight-row trip boundary (the lower row wins); with the prologue + ReLU the 17-row segment is all negative: value 0,
    its first row wins.  An empty segment: value 0, arg = N."""
    ops = _ops()
    g, sizes, bbd, ptr, N, P, plant = _segments()
    X = _segment_x(D)
    bx = Buf(N, [D])
    bx.slot(0).copy_(X.to(DEV))
    bx.snapshot()
    x_pro = gr.pro_scale_shift(D, 103 + D) if pro else None
    x_pro_d = tuple(t.to(DEV) for t in x_pro) if pro else None
    by = Buf(P, [D])
    by.snapshot()
    Y = by.slot(0)
    argb = torch.full((P + 1, D), -7, dtype=torch.int32, device=DEV)

    def run():
        Y.fill_(NAN)
        argb[:P].fill_(-7)
        ops.segment_max_fwd(bx.slot(0), g, Y, argb[:P], x_pro=x_pro_d, x_relu=pro)
        return (Y.clone(), argb[:P].clone())
    got, arg = _twice(run)
    assert by.untouched_outside([0]) and bx.untouched_outside([]) and bool((argb[P] == -7).all())
    v = X.numpy()
    if pro:
        v = np.maximum(gr.fma32(v, x_pro[0].numpy()[None, :], x_pro[1].numpy()[None, :]), np.float32(0))
    wx, wa = gr.first_argmax(v, ptr, N)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), wx.view(np.uint32))
    assert np.array_equal(arg.cpu().numpy(), wa.astype(np.int32))
    seg = lambda r: int(np.searchsorted(ptr, r, side="right") - 1)
    assert (wa[seg(plant["tie78"])] == plant["tie78"] + 7).all() and (wa[seg(plant["tie09"])] == plant["tie09"]).all()
    assert (wa[sizes == 0] == N).all() and (wx[sizes == 0] == 0).all()
    if pro:
        r0, _ = plant["negative"]
        assert (wx[seg(r0)] == 0).all() and (wa[seg(r0)] == r0).all()
    print("ratio %-18s %-12s exact" % ("segment_max_fwd D=%d" % D, "Y, arg"))


@pytest.mark.parametrize("D", gr.SEGMENT_D)
def test_segment_backward_matches_fp64_autograd_of_scatter(D):
    """ops.segment_mean_bwd and segment_max_bwd (D = 128, 1152: the float4 kernels; D = 5: the scalar ones) against float64
    autograd of the reference scatter (oracle_torch.scatter, reduce = mean / max) on the same fp32 X: the mean's gradient
    dY[p] / cnt within u |want| (one division), the max's EQUAL — dY where the row is the first argmax, 0 elsewhere."""
    from oracle import oracle_torch as orc
    ops = _ops()
    g, sizes, bbd, ptr, N, P, plant = _segments()
    X = _segment_x(D)
    Xd = X.to(DEV)
    bdy = Buf(P, [D])
    dY = gr.randn32((P, D), 104 + D)
    bdy.slot(0).copy_(dY.to(DEV))
    bdy.snapshot()
    bdx = Buf(N, [D])
    bdx.snapshot()
    dX = bdx.slot(0)
    Yx = torch.empty(P, D, device=DEV)
    arg = torch.empty(P, D, dtype=torch.int32, device=DEV)
    ops.segment_max_fwd(Xd, g, Yx, arg)
    bb = bbd.cpu()

    def run_mean():
        dX.fill_(NAN)
        ops.segment_mean_bwd(bdy.slot(0), g, dX)
        return (dX.clone(),)

    def run_max():
        dX.fill_(NAN)
        ops.segment_max_bwd(bdy.slot(0), arg, g, dX)
        return (dX.clone(),)
    got_mean, got_max = _twice(run_mean)[0], _twice(run_max)[0]
    assert bdx.untouched_outside([0]) and bdy.untouched_outside([])
    x64 = X.double().requires_grad_(True)
    orc.scatter(x64, bb, dim_size=P, reduce="mean").backward(dY.double())
    want = x64.grad.to(DEV)
    _worst("segment_mean_bwd D=%d" % D, "dX", got_mean, want, gr.segment_mean_bwd_tol(want))
    x64 = X.double().requires_grad_(True)
    orc.scatter(x64, bb, dim_size=P, reduce="max").backward(dY.double())
    assert torch.equal(got_max.double().cpu(), x64.grad)
    print("ratio %-18s %-12s exact" % ("segment_max_bwd D=%d" % D, "dX"))
