"""GPU tests (-m gpu) of the bf16-STORAGE training ops (include/yolat_hip.h "Training with bfloat16 STORAGE": the `_h`
entry points and the `half` instantiations) against float64 references at ragged shapes and hub graphs.

Every kernel here accumulates in fp32 and rounds to nearest even where it stores bfloat16, so every output has a tight
reference (tests/bf16_ref.py): the float64 value of the op on the bfloat16 inputs, an fp32 accumulation bound `delta`
formed from the operand magnitudes, and half a bfloat16 spacing on top for a bfloat16 output (store_envelope).  Nothing
is compared at a tensor's maximum.  Each test prints its worst error / tolerance ratio.

Conventions: operands live in column slots of wider buffers pre-filled with NaN (the way the training step lays its
[E,*] tensors out); after the call everything outside the output slots must hold the bits it held before; each op runs
twice and must return the same bits.  Inputs come from seeded CPU generators; the float64 references are evaluated on
the device."""
import numpy as np
import pytest
import torch

import bf16_ref as br

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
EPS32 = br.EPS32
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
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


class Buf(object):
    """[rows + 3, sum of the slot widths (each padded to 8 columns) + 8] NaN-filled buffer; slot(i) = rows x width view"""

    def __init__(self, rows, widths, dtype):
        self.rows, self.cols, c = rows, [], 0
        for w in widths:
            self.cols.append((c, c + w))
            c += -(-w // 8) * 8
        self.buf = torch.full((rows + 3, c + 8), NAN, dtype=dtype, device=DEV)
        self.snap = None

    def slot(self, i):
        lo, hi = self.cols[i]
        return self.buf[:self.rows, lo:hi]

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
        return torch.equal(_bits(self.buf)[mask], _bits(self.snap)[mask]) and bool(torch.isnan(self.buf[pad].float()).all())


def _vec(n, fill=NAN):
    """([n] view, [n + 8] buffer) fp32: the tail must stay NaN"""
    b = torch.full((n + 8,), NAN, dtype=torch.float32, device=DEV)
    b[:n] = fill
    return b[:n], b


def _tail_is_nan(b, n):
    return bool(torch.isnan(b[n:]).all())


def _worst(op, name, got, want, tol, where=None):
    """asserts |got - want| <= tol (elementwise, NaN fails) on `where`; prints and returns the worst error / tolerance"""
    err = (got.double() - want).abs()
    ok = err <= tol
    if where is not None:
        ok = ok | ~where
        err = torch.where(where, err, torch.zeros_like(err))
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("ratio %-18s %-12s %.3f" % (op, name, ratio))
    assert bool(ok.all()), "%s %s: %d of %d outside the tolerance, worst error / tolerance %.3f" % (
        op, name, int((~ok).sum()), ok.numel(), ratio)
    return ratio


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _check_stats(op, st, M, N, v, dv):
    """st: the flat fp32 statistics buffer (NaN-filled before the call); v / dv: float64 unrounded values and their bound"""
    G = (M + 31) // 32
    n = 2 * G * N
    got = st[:n].view(G, N, 2)
    s, m2, ts, tm = br.group_stats_ref(v, dv)
    _worst(op, "stats sum", got[:, :, 0], s, ts)
    _worst(op, "stats M2", got[:, :, 1], m2, tm)
    assert _tail_is_nan(st, n), "%s: statistics written past the last row group" % op


# ---------------------------------------------------------------------------------------------
# 1 / 2  the two Linears on the bf16 matrix cores
# ---------------------------------------------------------------------------------------------
LIN_SHAPES = [(1, 64, 64), (31, 64, 64), (33, 64, 64), (63, 64, 64), (65, 64, 64), (127, 64, 64), (4099, 64, 64),
              (300, 128, 64), (300, 64, 34), (97, 192, 130)]


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("pro", ["none", "affine", "relu"])
@pytest.mark.parametrize("M,K,Nout", LIN_SHAPES)
def test_linear_fwd_bf16_storage_matches_fp64_within_half_a_spacing(M, K, Nout, pro, with_stats):
    """ops.linear_fwd on bfloat16 A, Y (yolat_linear_fwd_h): Y = bf(pro(A)) . bf(W)^T + bias within store_envelope, delta
    = 2 (K + 2) 2^-24 (|a| . |w| + |bias|).  The prologue inputs lie on the exact grid (bf16_ref), without ReLU the floor
    is -inf.  Statistics: (sum, M2 about the group mean) per 32-row group of the UNROUNDED values, the last group short,
    nothing written past it; tolerances derived in bf16_ref.group_stats_ref from the same delta."""
    ops = _ops()
    seed = 7 * M + K + Nout
    A = br.grid_activation(M, K, seed)
    scale, shift = br.grid_scale_shift(K, seed + 1)
    W = _randn((Nout, K), seed + 2, 1 / 8).to(DEV)
    bias = _randn((Nout,), seed + 3, 0.1).to(DEV)
    b = Buf(M, [K, Nout], BF)
    b.slot(0).copy_(A.to(DEV))
    b.snapshot()
    a_pro = None if pro == "none" else (scale.to(DEV), shift.to(DEV))
    Y = b.slot(1)

    def run():
        Y.fill_(NAN)
        st = None
        if with_stats:
            st = ops.stats_buffer(M, Nout, DEV)
            st.fill_(NAN)
        ops.linear_fwd(b.slot(0), W, bias, Y, a_pro=a_pro, a_relu=pro == "relu", stats=st)
        return Y.clone(), st
    y1, st1 = run()
    y2, st2 = run()
    assert torch.equal(_bits(y1), _bits(y2))
    assert b.untouched_outside([1])
    sc, sh = a_pro if a_pro is not None else (None, None)
    want, delta = br.linear_fwd_ref(b.slot(0), sc, sh, pro == "relu", W, bias)
    _worst("linear_fwd_h", "Y", y1, want, br.store_envelope(want, delta))
    if with_stats:
        assert torch.equal(_bits(st1), _bits(st2))
        _check_stats("linear_fwd_h", st1, M, Nout, want, delta)


@pytest.mark.parametrize("M,K,Nout", LIN_SHAPES)
def test_linear_fwd_wt_bf16_storage_matches_fp64_within_half_a_spacing(M, K, Nout):
    """ops.linear_fwd_wt on bfloat16 (yolat_linear_fwd_wt_h): Y = dY . bf(Wt) within store_envelope."""
    ops = _ops()
    seed = 11 * M + K + Nout
    A = _randn((M, K), seed).to(BF)
    Wt = _randn((K, Nout), seed + 1, 1 / 8).to(DEV)
    b = Buf(M, [K, Nout], BF)
    b.slot(0).copy_(A.to(DEV))
    b.snapshot()
    Y = b.slot(1)
    outs = []
    for _ in range(2):
        Y.fill_(NAN)
        ops.linear_fwd_wt(b.slot(0), Wt, Y)
        outs.append(Y.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert b.untouched_outside([1])
    a, wb = b.slot(0).double(), br.bf(Wt)
    want = a @ wb
    _worst("linear_fwd_wt_h", "Y", outs[0], want, br.store_envelope(want, br.dot_delta(a.abs() @ wb.abs(), K)))


# ---------------------------------------------------------------------------------------------
# 3  weight gradient with bfloat16 dY
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("Nout,K,amode", [(64, 64, "bf16"), (64, 64, "bf16_pro"), (64, 64, "fp32"), (64, 4, "fp32")])
@pytest.mark.parametrize("M", [1, 33, 1000, 70001])
def test_linear_bwd_w_bf16_storage_matches_fp64(M, Nout, K, amode, with_db, accumulate):
    """ops.linear_bwd_w with bfloat16 dY (yolat_linear_bwd_w_h): dW (+)= dY^T . pro(A), db (+)= column sums, fp32
    outputs: |error| <= 2 (M + 2) 2^-24 |dY|^T . |pro(A)| (+ one rounding of the accumulating addition).  The prologue
    of this kernel stays in fp32 (HalfProOp: no re-rounding); its inputs lie on the exact grid.  (64, 4) with fp32 A is
    the fall-back of ops.attr_dw.  M = 70001 runs 438 row splits of 160 rows (yl_tn_plan: 1024 / tiles = 512 wanted
    splits, ceil(70001 / 512) = 137 rounded up to a multiple of 32), M = 1000 sixteen of 64, M <= 64 one: the scratch
    size states the split count."""
    ops = _ops()
    lib, _ = _lib()
    seed = 13 * M + K + 2 * len(amode)
    dY = _randn((M, Nout), seed).to(BF)
    by = Buf(M, [Nout], BF)
    by.slot(0).copy_(dY.to(DEV))
    by.snapshot()
    a_pro, a_relu = None, False
    if amode == "fp32":
        ba = Buf(M, [K], torch.float32)
        ba.slot(0).copy_(_randn((M, K), seed + 1).to(DEV))
        pa = ba.slot(0).double()
    else:
        ba = Buf(M, [K], BF)
        ba.slot(0).copy_(br.grid_activation(M, K, seed + 1).to(DEV))
        pa = ba.slot(0).double()
        if amode == "bf16_pro":
            scale, shift = br.grid_scale_shift(K, seed + 2)
            a_pro, a_relu = (scale.to(DEV), shift.to(DEV)), True
            assert br.prologue_is_exact_in_fp32(ba.slot(0), a_pro[0], a_pro[1])
            pa = br.prologue(ba.slot(0), a_pro[0], a_pro[1], True)
    ba.snapshot()
    splits = int(lib.yolat_linear_bwd_w_work_elems(M, Nout, K)) // (Nout * K + Nout)
    assert splits == {1: 1, 33: 1, 1000: 16, 70001: 438}[M]
    bw = Buf(Nout, [K], torch.float32)
    base_w = _randn((Nout, K), seed + 3).to(DEV)
    base_b = _randn((Nout,), seed + 4).to(DEV)
    dW = bw.slot(0)
    outs = []
    for _ in range(2):
        dW.copy_(base_w if accumulate else torch.full_like(base_w, NAN))
        db, db_buf = _vec(Nout)
        if accumulate:
            db.copy_(base_b)
        bw.snapshot()
        ops.linear_bwd_w(by.slot(0), ba.slot(0), dW, db if with_db else None, a_pro=a_pro, a_relu=a_relu,
                         accumulate=accumulate)
        assert bw.untouched_outside([0]) and _tail_is_nan(db_buf, Nout)
        outs.append((dW.clone(), db.clone()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert by.untouched_outside([]) and ba.untouched_outside([])
    y = by.slot(0).double()
    want_w, tol_w = y.t() @ pa, 2.0 * (M + 2) * EPS32 * (y.abs().t() @ pa.abs())
    want_b, tol_b = y.sum(0), 2.0 * (M + 2) * EPS32 * y.abs().sum(0)
    if accumulate:
        tol_w = tol_w + EPS32 * (base_w.double().abs() + want_w.abs())
        tol_b = tol_b + EPS32 * (base_b.double().abs() + want_b.abs())
        want_w, want_b = want_w + base_w.double(), want_b + base_b.double()
    _worst("linear_bwd_w_h", "dW", outs[0][0], want_w, tol_w)
    if with_db:
        _worst("linear_bwd_w_h", "db", outs[0][1], want_b, tol_b)
    else:
        assert torch.equal(_bits(outs[0][1]), _bits(base_b if accumulate else torch.full_like(base_b, NAN)))


# ---------------------------------------------------------------------------------------------
# 4  BatchNorm + ReLU backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", [1, 63, 65, 1000, 262144 + 70])
def test_bn_relu_bwd_bf16_storage_matches_fp64(M, C, relu, accumulate):
    """ops.bn_relu_bwd (yolat_bn_relu_bwd_h) and ops.bn_relu_bwd_apply (half = 1) on bfloat16 dZ / Y / dY against the
    float64 restatement dY = scale (dZ [z > 0] - c1 - xhat c2) with REAL batch statistics (bf16_ref.bn_bwd_inputs).
    M = 262144 + 70 is past the 4096 x 64 rows the apply kernel's grid covers in one sweep: its row loop runs.

    Elements with |z| <= 1e-4 may be masked either way in fp32: they are left out of the dY comparison (at most 0.1 %
    of the elements: a condition on the inputs, checked on the CPU in test_bf16_ref_host.py and again here) and enter
    the tolerances of the sums with their full magnitude.
    Sums (dgamma = sum g xhat, dbeta = sum g): fp32 over blocks of 512 rows, fp64 across blocks, one rounding to fp32:
        |error| <= (min(M, 512) + 6) 2^-24 sum |terms|   (3 roundings inside a term, the block's additions, the final one)
    dY: six fp32 roundings in  a (g - k1 - ((y - m) i) k2), each relative to an intermediate no larger than
        S = |scale| (|g| + |c1| + |xhat c2|):  delta = 8 2^-24 S  (6 to first order, 8 covers the second);
    bn_relu_bwd forms (c1, c2) itself: their error (the sums' tolerance / M) is added as |scale| (dc1 + |xhat| dc2);
    bn_relu_bwd_apply is GIVEN (c1, c2) as fp32 vectors and the reference uses those very values."""
    ops = _ops()
    seed = M + C
    Y, dZ, mean, invstd, scale, shift = br.bn_bwd_inputs(M, C, seed)
    mean, invstd, scale, shift = [t.to(DEV) for t in (mean, invstd, scale, shift)]
    b = Buf(M, [C, C, C], BF)
    b.slot(0).copy_(dZ.to(DEV))
    b.slot(1).copy_(Y.to(DEV))
    b.snapshot()
    dZd, Yd, dY = b.slot(0), b.slot(1), b.slot(2)
    base_g, base_b = _randn((C,), seed + 1).to(DEV), _randn((C,), seed + 2).to(DEV)
    outs = []
    for _ in range(2):
        dY.fill_(NAN)
        dg, dg_buf = _vec(C)
        dbt, dbt_buf = _vec(C)
        if accumulate:
            dg.copy_(base_g)
            dbt.copy_(base_b)
        ops.bn_relu_bwd(dZd, Yd, scale, mean, invstd, scale, shift, relu, dg, dbt, dY, accumulate=accumulate)
        assert _tail_is_nan(dg_buf, C) and _tail_is_nan(dbt_buf, C)
        outs.append((dY.clone(), dg.clone(), dbt.clone()))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(_bits(x), _bits(y))
    assert b.untouched_outside([2])
    ref = br.bn_relu_bwd_ref(dZd, Yd, mean, invstd, scale, shift, relu)
    sure, g, xhat = ref["sure"], ref["g"], ref["xhat"]
    unsure = (~sure).double()
    assert float(unsure.mean()) <= br.KINK_SHARE
    n_blk = min(M, 512)
    tol_b = (n_blk + 6) * EPS32 * g.abs().sum(0) + (dZd.double().abs() * unsure).sum(0)
    tol_g = (n_blk + 6) * EPS32 * (g * xhat).abs().sum(0) + ((dZd.double() * xhat).abs() * unsure).sum(0)
    dc1, dc2 = tol_b / M, tol_g / M
    want_g, want_b = ref["dgamma"], ref["dbeta"]
    acc_g, acc_b = torch.zeros_like(tol_g), torch.zeros_like(tol_b)
    if accumulate:
        acc_g = EPS32 * (base_g.double().abs() + want_g.abs())
        acc_b = EPS32 * (base_b.double().abs() + want_b.abs())
        want_g, want_b = want_g + base_g.double(), want_b + base_b.double()
    _worst("bn_relu_bwd_h", "dgamma", outs[0][1], want_g, tol_g + acc_g)
    _worst("bn_relu_bwd_h", "dbeta", outs[0][2], want_b, tol_b + acc_b)
    sc = scale.double().abs()
    S = sc * (g.abs() + ref["c1"].abs() + (xhat * ref["c2"]).abs())
    delta = 8.0 * EPS32 * S + sc * (dc1 + xhat.abs() * dc2)
    _worst("bn_relu_bwd_h", "dY", outs[0][0], ref["dY"], br.store_envelope(ref["dY"], delta), sure)
    del S, delta
    # ---- the apply pass alone, coefficients given
    coef = torch.cat([ref["c1"], ref["c2"]]).float()
    ref2 = br.bn_relu_bwd_ref(dZd, Yd, mean, invstd, scale, shift, relu, coef=coef)
    outs = []
    for _ in range(2):
        dY.fill_(NAN)
        ops.bn_relu_bwd_apply(dZd, Yd, mean, invstd, scale, shift, relu, coef, dY)
        outs.append(dY.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert b.untouched_outside([2])
    delta = 8.0 * EPS32 * sc * (g.abs() + ref2["c1"].abs() + (xhat * ref2["c2"]).abs())
    _worst("bn_relu_bwd_apply", "dY", outs[0], ref2["dY"], br.store_envelope(ref2["dY"], delta), sure)


# ---------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------
GRAPHS = {
    "tiny": lambda: (20,) + br.uniform(20, 7, seed=1),                    # E < 32
    "hub65": lambda: (300,) + br.hub(300, 2000, 65, seed=2),
    "hub150": lambda: (300,) + br.hub(300, 2000, 150, seed=3),
    "hub1000": lambda: (300,) + br.hub(300, 2000, 1000, seed=4),
    "chain257": lambda: (257,) + br.chain(257),
    "uniform": lambda: (40000,) + br.uniform(40000, 9000, seed=5),
}


def _graph(N, src, dst, seed=0):
    """(ops.Graph, CSR-ordered src / dst int64 device tensors, CSR-ordered attr) — the CSR order is derived with numpy
    (stable sort by destination) and the prepared graph is checked against it"""
    ops = _ops()
    E = len(src)
    attr = np.random.default_rng(seed + E).standard_normal((E, 4)).astype(np.float32) * 0.5
    g = ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).to(DEV), torch.from_numpy(attr).to(DEV), None, N, 1)
    g.check_status()
    order = np.argsort(dst, kind="stable")
    s, d, a = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (src[order], dst[order], attr[order]))
    assert torch.equal(g.src[:E].long(), s) and torch.equal(g.dst[:E].long(), d) and torch.equal(g.attr[:E], a)
    rp = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))])
    assert torch.equal(g.row_ptr.long().cpu(), torch.from_numpy(rp))
    return g, s, d, a


# ---------------------------------------------------------------------------------------------
# 5 / 6  mean aggregation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "pro", "acc", "pro_acc"])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_csr_mean_fwd_bf16_storage_matches_fp64(graph, mode):
    """ops.csr_mean_fwd on bfloat16 H (yolat_csr_mean_fwd_h): out (+)= mean over the CSR row of pro(H), fp32 output.
    pro = the BatchNorm + ReLU prologue on the exact grid (an fp32 fma, not re-rounded here).  Tolerance per node and
    column: a sum of deg fp32 additions, the rounded reciprocal of deg and the rounded product,
        (deg + 3) 2^-24 sum |pro(h)| / deg,   + 2^-24 (|base| + |mean|) for the accumulating addition.
    A node without in-edge: the base bit for bit when accumulating, else exactly 0."""
    ops = _ops()
    N, src, dst = GRAPHS[graph]()
    E = len(src)
    g, s, d, _ = _graph(N, src, dst)
    seed = N + E
    pro, acc = mode.startswith("pro"), mode.endswith("acc")
    bh = Buf(E, [64], BF)
    bh.slot(0).copy_((br.grid_activation(E, 64, seed) if pro else _randn((E, 64), seed).to(BF)).to(DEV))
    bh.snapshot()
    h_pro = None
    hv = bh.slot(0).double()
    if pro:
        scale, shift = br.grid_scale_shift(64, seed + 1)
        h_pro = (scale.to(DEV), shift.to(DEV))
        hv = br.prologue(bh.slot(0), h_pro[0], h_pro[1], True)
    bo = Buf(N, [64], torch.float32)
    base = (_randn((N, 64), seed + 2) + 3.0).to(DEV)                   # non-zero everywhere
    out = bo.slot(0)
    outs = []
    for _ in range(2):
        out.copy_(base if acc else torch.full_like(base, NAN))
        bo.snapshot()
        ops.csr_mean_fwd(bh.slot(0), g, out, h_pro=h_pro, h_relu=pro, accumulate=acc)
        assert bo.untouched_outside([0])
        outs.append(out.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert bh.untouched_outside([])
    mean, mag, deg = br.csr_mean_ref(hv, d, N)
    tol = (deg[:, None] + 3.0) * EPS32 * mag / deg.clamp_min(1)[:, None]
    want = mean
    if acc:
        tol = tol + EPS32 * (base.double().abs() + mean.abs())
        want = mean + base.double()
    _worst("csr_mean_fwd_h", "out", outs[0], want, tol)
    empty = deg == 0
    assert bool(empty.any()) or graph == "chain257"
    if acc:
        assert torch.equal(_bits(outs[0][empty]), _bits(base[empty]))
    else:
        assert bool((outs[0][empty] == 0).all())


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_csr_mean_bwd_bf16_storage_is_the_rounded_quotient(graph):
    """ops.csr_mean_bwd to bfloat16 (yolat_csr_mean_bwd_h): dM[q] = bf(dOut[dst_q] / deg).

    The kernel multiplies by the fp32 reciprocal fl(1 / deg) and rounds the product to fp32 before the bfloat16 store
    (k_csr_mean_bwd_v4; the header's contract names the quotient only) — two roundings of 2^-24 in front of the store.
    So: (a) BIT equality with that arithmetic done in fp32 by torch (IEEE division and product, torch's conversion: the
    standard of test_bf16_storage_ops_round_to_nearest_even...), and (b) equality with the float64 bf(dOut / deg)
    everywhere except where the exact quotient lies within those two roundings (2 x 2^-24 |q|, i.e. 2^-15 of a bfloat16
    spacing at most) of a rounding boundary — there the neighbouring bfloat16 value is the only other answer."""
    ops = _ops()
    N, src, dst = GRAPHS[graph]()
    E = len(src)
    g, s, d, _ = _graph(N, src, dst)
    bo = Buf(N, [64], torch.float32)
    bo.slot(0).copy_(_randn((N, 64), N + E + 9).to(DEV))
    bo.snapshot()
    bm = Buf(E, [64], BF)
    bm.snapshot()
    dM = bm.slot(0)
    outs = []
    for _ in range(2):
        dM.fill_(NAN)
        ops.csr_mean_bwd(bo.slot(0), g, dM)
        outs.append(dM.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert bm.untouched_outside([0]) and bo.untouched_outside([])
    deg = torch.bincount(d, minlength=N).clamp_min(1)
    inv = (1.0 / deg.cpu().float()).to(DEV)                           # IEEE division
    emu = (bo.slot(0)[d] * inv[d][:, None]).to(BF)
    assert torch.equal(_bits(outs[0]), _bits(emu))
    q = br.csr_mean_bwd_ref(bo.slot(0), d, N)
    want = br.bf(q)
    u = br.ulp_bf16(q)
    frac = q.abs() / u - torch.floor(q.abs() / u)
    near_tie = (frac - 0.5).abs() <= 2.0 * EPS32 * q.abs() / u * (1 + 2.0 ** -20)
    diff = (outs[0].double() - want).abs()
    assert bool(((diff == 0) | (near_tie & (diff <= u))).all())
    print("ratio %-18s %-12s %d of %d elements on a rounding boundary" % ("csr_mean_bwd_h", "dM", int((diff != 0).sum()),
                                                                       diff.numel()))
    assert float((diff != 0).double().mean()) <= 2.0 ** -12


# ---------------------------------------------------------------------------------------------
# 7  factorised first edge Linear
# ---------------------------------------------------------------------------------------------
EDGE_CASES = [(1, "uniform"), (31, "uniform"), (33, "uniform"), (63, "uniform"), (64, "uniform"), (65, "uniform"),
              (1000, "uniform"), (4097, "uniform"), (1000, "hub150"), (4097, "hub1000")]


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("with_b1", [False, True])
@pytest.mark.parametrize("E,kind", EDGE_CASES)
def test_edge_uv_lin1_fwd_bf16_storage_matches_fp64(E, kind, with_b1, with_stats):
    """yolat_edge_uv_lin1_fwd_h through the library with a GIVEN fp32 UV: H1[q] = U[dst_q] + V[src_q] + Wc4 . attr_q + b1
    stored as bfloat16.  k_edge_uv_lin1 rounds six times (u + v, four fmas, + b1), each relative to a partial sum no
    larger than S = |u| + |v| + |attr| . |Wc4| + |b1|:  delta = 6 2^-24 S.  Statistics of the unrounded values as in the
    Linear.  A hub graph needs E >= 2 deg: hub150 at E = 1000, hub1000 at E = 4097; below that the graph is uniform."""
    ops = _ops()
    lib, check = _lib()
    if kind == "uniform":
        N = 50
        src, dst = br.uniform(N, E, seed=E)
    else:
        N = 300
        src, dst = br.hub(N, E, int(kind[3:]), seed=E)
    g, s, d, attr = _graph(N, src, dst)
    seed = 3 * E + N
    buv = Buf(N, [128], torch.float32)
    buv.slot(0).copy_(_randn((N, 128), seed).to(DEV))
    buv.snapshot()
    wc4 = _randn((64, 4), seed + 1, 0.5).to(DEV)
    b1 = _randn((64,), seed + 2, 0.3).to(DEV) if with_b1 else None
    bh = Buf(E, [64], BF)
    bh.snapshot()
    H1, UV = bh.slot(0), buv.slot(0)
    outs = []
    for _ in range(2):
        H1.fill_(NAN)
        st = None
        if with_stats:
            st = ops.stats_buffer(E, 64, DEV)
            st.fill_(NAN)
        check(lib.yolat_edge_uv_lin1_fwd_h(UV.data_ptr(), UV.stride(0), g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                           E, wc4.data_ptr(), b1.data_ptr() if with_b1 else None, 64, H1.data_ptr(),
                                           H1.stride(0), st.data_ptr() if with_stats else None, _stream()),
              "yolat_edge_uv_lin1_fwd_h")
        outs.append((H1.clone(), st))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    assert bh.untouched_outside([0]) and buv.untouched_outside([])
    U, V = UV[:, :64].double(), UV[:, 64:].double()
    bb = b1.double() if with_b1 else torch.zeros(64, dtype=torch.float64, device=DEV)
    want = U[d] + V[s] + attr.double() @ wc4.double().t() + bb
    S = U[d].abs() + V[s].abs() + attr.double().abs() @ wc4.double().abs().t() + bb.abs()
    delta = 6.0 * EPS32 * S * (1 + 2.0 ** -20)
    _worst("edge_uv_lin1_fwd_h", "H1", outs[0][0], want, br.store_envelope(want, delta))
    if with_stats:
        assert torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        _check_stats("edge_uv_lin1_fwd_h", outs[0][1], E, 64, want, delta)


# ---------------------------------------------------------------------------------------------
# 8  BatchNorm + ReLU + mean aggregation backward, never materialised
# ---------------------------------------------------------------------------------------------
# the last two: 513 and 1025 tiles, i.e. two and three per workgroup of the one-kernel backward (512 workgroups at most), the
# last workgroup one and two — the smallest E at which its two-tiles-in-flight pipeline and cross-tile accumulators run
BN_CSR_CASES = [(50, 31, "uniform"), (64, 64, "uniform"), (64, 65, "uniform"), (64, 129, "uniform"), (300, 1000, "uniform"),
                (300, 1000, "hub150"), (4000, 32769, "uniform"), (4000, 65537, "hub1000")]


def _bn_csr_case(N, E, kind):
    ops = _ops()
    src, dst = br.uniform(N, E, seed=N + E) if kind == "uniform" else br.hub(N, E, int(kind[3:]), seed=N + E)
    g, s, d, _ = _graph(N, src, dst)
    seed = 5 * N + E
    Y, _, mean, invstd, scale, shift = br.bn_bwd_inputs(E, 64, seed)
    coefs = [t.to(DEV) for t in (mean, invstd, scale, shift)]
    b = Buf(E, [64, 64, 64], BF)                                      # Y | A | dA
    b.slot(0).copy_(Y.to(DEV))
    b.slot(1).copy_(br.grid_activation(E, 64, seed + 1).to(DEV))
    b.snapshot()
    bo = Buf(N, [64], torch.float32)
    bo.slot(0).copy_(_randn((N, 64), seed + 2).to(DEV))
    bo.snapshot()
    asc, ash = (t.to(DEV) for t in br.grid_scale_shift(64, seed + 3))
    W = _randn((64, 64), seed + 4, 1 / 8).to(DEV)
    return ops, g, d, coefs, b, bo, (asc, ash), W, seed


@pytest.mark.parametrize("with_next", [False, True])
@pytest.mark.parametrize("N,E,kind", BN_CSR_CASES)
def test_bn_csr_grad_bf16_storage_matches_fp64(N, E, kind, with_next):
    """ops.BnCsrGrad with bfloat16 Y (bn_csr.hip): stats(), then bwd_w_and_x() on bfloat16 A / dA (k_bn_csr_l2_bwd_h),
    with and without the statistics of the next BatchNorm's backward.  31 and 64 edges are one 64-row tile, 129 three
    (an odd count for the kernel that keeps two tiles in flight); hub150 puts a 150-edge segment over three tiles and
    130 nodes without in-edge behind it (a hub needs E >= 2 deg: of the small cases only (300, 1000) can hold one).
    32769 and 65537 edges are 513 and 1025 tiles: two and three per workgroup, the last workgroup one and two, so the
    two-tiles-in-flight pipeline, the prefetch two tiles ahead and the accumulators carried from tile to tile all run.

    Reference: the float64 backward of mean-aggregate(relu(batchnorm(Y))) on the bfloat16 values of Y, restated as
    dY = scale (g - c1 - xhat c2) with g = [z > 0] d_out[dst] / deg (bf16_ref.bn_relu_bwd_ref is checked against autograd
    in test_bf16_ref_host.py).  Tolerances, per output:
      dgamma, dbeta, (c1, c2) = sums / E: fp32 over blocks of 640 rows, fp64 across; a term carries two more roundings
          than in bn_relu_bwd (fl(1 / deg) and the product):  (min(E, 640) + 8) 2^-24 sum |terms|, + the full magnitude
          of the terms within 1e-4 of the ReLU kink (at most 0.1 % of the elements).
      dY (never stored; formed in fp32 from the kernel's OWN fp32 (c1, c2), which the reference takes over):
          d_dY = 10 2^-24 |scale| (|g| + |c1| + |xhat c2|)  (eight as in bn_relu_bwd + the two of g), + |scale g| on the kink.
      The one-kernel form rounds dY, relu(bn(A)) (exact grid: no ambiguity) and W to bfloat16 for the matrix cores:
          r_dY = store_envelope(dY, d_dY) per element.
      dW = dY^T . bf(A1):   r_dY^T . |A1| + 2 (E + 2) 2^-24 |dY|^T . |A1|
      db = column sums of the fp32 dY:   sum d_dY + (E + 2) 2^-24 sum |dY|
      dA = bf16 store of dY . bf(W):   store_envelope(dA, r_dY . |bf W| + 2 (64 + 2) 2^-24 |dY| . |bf W|)
      next BatchNorm (dgamma, dbeta, coefficients): float64 sums of the kernel's STORED dA (its contract: "the statistics
          take the stored values"), masked by the exact grid prologue of A; fp32 over one workgroup's 64 ceil(tiles / 512)
          rows, fp64 across:  (64 ceil(tiles / 512) + 6) 2^-24 sum |terms|."""
    ops, g, d, (mean, invstd, scale, shift), b, bo, (asc, ash), W, seed = _bn_csr_case(N, E, kind)
    Y, A, dA = b.slot(0), b.slot(1), b.slot(2)
    m1 = _randn((64,), seed + 5, 0.2).to(DEV)
    is1 = (torch.rand(64, generator=torch.Generator().manual_seed(seed + 6)) + 0.5).to(DEV)

    def run():
        dA.fill_(NAN)
        dg, dg_buf = _vec(64)
        dbt, dbt_buf = _vec(64)
        dbias, dbias_buf = _vec(64)
        ng, ng_buf = _vec(64)
        nb, nb_buf = _vec(64)
        bw = Buf(64, [64], torch.float32)
        bw.snapshot()
        h = ops.BnCsrGrad(bo.slot(0), g, Y, mean, invstd, scale, shift, relu=True)
        h.stats(dg, dbt)
        coef = h.coef.clone()
        coef1 = h.bwd_w_and_x(A, W, bw.slot(0), dbias, dA, a_pro=(asc, ash), a_relu=True,
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
    got = run()
    for x, y in zip(got, run()):
        assert torch.equal(_bits(x), _bits(y))
    assert b.untouched_outside([2]) and bo.untouched_outside([])
    dg, dbt, coef, dW, dbias, dA_got = got[:6]
    # ---- statistics
    g0 = br.csr_mean_bwd_ref(bo.slot(0), d, N)
    ref = br.bn_relu_bwd_ref(g0, Y, mean, invstd, scale, shift, True)
    unsure = (~ref["sure"]).double()
    assert float(unsure.mean()) <= br.KINK_SHARE
    xhat = ref["xhat"]
    n_blk = min(E, 640)
    tol_b = (n_blk + 8) * EPS32 * ref["g"].abs().sum(0) + (g0.abs() * unsure).sum(0)
    tol_g = (n_blk + 8) * EPS32 * (ref["g"] * xhat).abs().sum(0) + ((g0 * xhat).abs() * unsure).sum(0)
    _worst("bn_csr_bwd_stats", "dgamma", dg, ref["dgamma"], tol_g)
    _worst("bn_csr_bwd_stats", "dbeta", dbt, ref["dbeta"], tol_b)
    _worst("bn_csr_bwd_stats", "c1", coef[:64], ref["c1"], tol_b / E)
    _worst("bn_csr_bwd_stats", "c2", coef[64:], ref["c2"], tol_g / E)
    # ---- the one-kernel consumers, dY formed from the kernel's own coefficients
    ref = br.bn_relu_bwd_ref(g0, Y, mean, invstd, scale, shift, True, coef=coef)
    dY, sc = ref["dY"], scale.double().abs()
    d_dY = 10.0 * EPS32 * sc * (ref["g"].abs() + ref["c1"].abs() + (xhat * ref["c2"]).abs()) + sc * g0.abs() * unsure
    r_dY = br.store_envelope(dY, d_dY)
    assert br.prologue_is_exact_in_fp32(A, asc, ash)
    A1 = br.bf(br.prologue(A, asc, ash, True))
    Wb = br.bf(W)
    _worst("bn_csr_l2_bwd", "dW", dW, dY.t() @ A1, r_dY.t() @ A1.abs() + 2.0 * (E + 2) * EPS32 * (dY.abs().t() @ A1.abs()))
    _worst("bn_csr_l2_bwd", "db", dbias, dY.sum(0), d_dY.sum(0) + (E + 2) * EPS32 * dY.abs().sum(0))
    want_dA = dY @ Wb
    d_dA = r_dY @ Wb.abs() + br.dot_delta(dY.abs() @ Wb.abs(), 64)
    _worst("bn_csr_l2_bwd", "dA", dA_got, want_dA, br.store_envelope(want_dA, d_dA))
    if with_next:
        ng, nb, coef1 = got[6:]
        z1 = br.prologue(A, asc, ash, False)                          # exact: the mask has no kink
        gp = dA_got.double() * (z1 > 0)
        xh1 = (A.double() - m1.double()) * is1.double()
        tiles = -(-E // 64)
        rows = 64 * -(-tiles // 512)
        t1 = (rows + 6) * EPS32 * gp.abs().sum(0)
        t2 = (rows + 6) * EPS32 * (gp * xh1).abs().sum(0)
        _worst("bn_csr_l2_bwd", "next dbeta", nb, gp.sum(0), t1)
        _worst("bn_csr_l2_bwd", "next dgamma", ng, (gp * xh1).sum(0), t2)
        _worst("bn_csr_l2_bwd", "next c1", coef1[:64], gp.sum(0) / E, t1 / E)
        _worst("bn_csr_l2_bwd", "next c2", coef1[64:], (gp * xh1).sum(0) / E, t2 / E)


def test_bn_csr_grad_two_kernel_consumers_refuse_bf16_storage():
    """BnCsrGrad.bwd_w / fwd_wt (yolat_linear_bwd_w_csr / yolat_linear_fwd_wt_csr) have NO bfloat16 form: with bfloat16 Y
    they return YOLAT_E_UNSUPPORTED (bn_csr.hip: "bfloat16 storage: yolat_bn_csr_l2_bwd only") — an error, not a quiet
    fp32 reading of bfloat16 bits — and leave their outputs alone."""
    from yolat_vectorgraphicsrecognition_amd._lib import YolatLibraryError
    ops, g, d, (mean, invstd, scale, shift), b, bo, (asc, ash), W, seed = _bn_csr_case(300, 1000, "uniform")
    h = ops.BnCsrGrad(bo.slot(0), g, b.slot(0), mean, invstd, scale, shift, relu=True)
    dg, dbt = torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    h.stats(dg, dbt)
    A32 = b.slot(1).float()
    dW = torch.full((64, 64), NAN, device=DEV)
    dA = torch.full((1000, 64), NAN, device=DEV)
    with pytest.raises(YolatLibraryError):
        h.bwd_w(A32, dW, None, a_pro=(asc, ash), a_relu=True)
    with pytest.raises(YolatLibraryError):
        h.fwd_wt(W, dA)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(dA).all())
