"""GPU tests, op level: the eval fusion pair with the GEMM emulated by three half-precision products (csrc/fusion_f16x3.hip
k_fusion_rows_f16x3, csrc/f16x3.hpp) against float64 and against the bf16x6 entry point on the same operands.

  yolat_split_f16x2                  the scaled two-term split alone: exponents, residual, zero / denormal rows
  yolat_fusion_pair_eval_f16x3       pooled[p] = max over the rows of proposal p of relu(A (s W)^T + t); the super half
  yolat_fusion_pair_eval_f16x3_act   the same for act(y) = y > 0 ? y : a y, both signs of a

Bars (those of tests/test_gpu_ops.py::test_fusion_x6_matches_fp32_fusion_kernel): worst error against float64 <= 2e-6 of the
output's largest magnitude, against the bf16x6 entry <= 3e-6 of it, two runs bit-identical, the super half under the same
bars.  The float64 reference multiplies the SAME fp32 operands (the scaled weights fl(s W) and the folded shift).

Shapes: N in {1, 33, 257, 600} (one row; a wave boundary; one row past a 256-row tile; a partial third tile), F in {64, 192}
(one and three column tiles), D in {64, 128} (both instantiations), and three proposal layouts: all rows in one proposal
(the run crosses waves and tiles), every row its own proposal, runs that end exactly at rows 31, 32, 255 and 256.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL64, TOLX6 = 2e-6, 3e-6
NS, FS, DS, LAYOUTS = (1, 33, 257, 600), (64, 192), (64, 128), ("one", "each", "edges")


def _seg(N, layout):
    """proposal id per row (non-decreasing, every proposal non-empty)"""
    if layout == "one":
        return np.zeros(N, dtype=np.int32)
    if layout == "each":
        return np.arange(N, dtype=np.int32)
    ends = sorted(set(e for e in (31, 32, 255, 256, N - 1) if e < N))
    seg, lo = np.zeros(N, dtype=np.int32), 0
    for p, e in enumerate(ends):
        seg[lo:e + 1] = p
        lo = e + 1
    return seg


def _act(y, a):
    return torch.relu(y) if a is None else torch.where(y > 0, y, a * y)


_CASES = {}


def _case(N, F, D, layout):
    """Operands (fp32, on the CPU) of one shape, built once and shared by the ReLU and the two leaky runs."""
    key = (N, F, D, layout)
    if key in _CASES:
        return _CASES[key]
    tg = torch.Generator().manual_seed(1000 * N + 10 * F + D + len(layout))
    seg = _seg(N, layout)
    P = int(seg[-1]) + 1
    A = torch.randn(N, D, generator=tg)
    A[N // 2] = 0.0                                              # an all-zero row
    S = torch.randn(P, D, generator=tg)
    S[P // 2] = 0.0
    W, Ws = torch.randn(F, D, generator=tg) / D ** 0.5, torch.randn(F, D, generator=tg) / D ** 0.5
    b, bs = torch.randn(F, generator=tg) * 0.1, torch.randn(F, generator=tg) * 0.1
    s, ss = torch.rand(F, generator=tg) - 0.25, torch.rand(F, generator=tg) - 0.25     # about a quarter negative
    t, ts = torch.randn(F, generator=tg) * 0.2, torch.randn(F, generator=tg) * 0.2
    s[2], t[2] = 0.05, -4.0                                      # column 2: negative in every row
    Wsc, Wssc = (W * s[:, None]).contiguous(), (Ws * ss[:, None]).contiguous()      # fl(s W): what both splits split
    tfold, tsfold = s * b + t, ss * bs + ts
    y = A.double() @ Wsc.double().t() + tfold.double()
    assert bool((y[:, 2] < 0).all())
    ys = S.double() @ Wssc.double().t() + tsfold.double()
    c = dict(N=N, F=F, D=D, P=P, seg=seg, A=A, S=S, W=W, Ws=Ws, s=s, ss=ss, tfold=tfold, tsfold=tsfold, y=y, ys=ys)
    _CASES[key] = c
    return c


def _run_pair(c, slope, emul):
    """pooled [P, F] and super [P, F] of one entry point (emul 'f16x3' | 'x6'), slope None: ReLU"""
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    N, F, D, P = c["N"], c["F"], c["D"], c["P"]
    dev = "cuda"
    A, S = c["A"].to(dev), c["S"].to(dev)
    W, Ws, s, ss = c["W"].to(dev), c["Ws"].to(dev), c["s"].to(dev), c["ss"].to(dev)
    tfold, tsfold = c["tfold"].to(dev), c["tsfold"].to(dev)
    seg = torch.from_numpy(c["seg"]).to(dev)
    seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(c["seg"], minlength=P))]).astype(np.int32)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    split = ops.split_f16x2 if emul == "f16x3" else ops.split_bf16x3
    wf, wfs = split(W, s), split(Ws, ss)
    p = lambda parts: [x.data_ptr() for x in parts]
    pool, Ys = torch.zeros(P, F, device=dev), torch.full((P, F), float("nan"), device=dev)
    if slope is None:
        fn = lib.yolat_fusion_pair_eval_f16x3 if emul == "f16x3" else lib.yolat_fusion_pair_eval_x6
        check(fn(A.data_ptr(), D, N, D, *p(wf), tfold.data_ptr(), F, seg.data_ptr(), pool.data_ptr(), F, S.data_ptr(), D, P,
                 *p(wfs), tsfold.data_ptr(), Ys.data_ptr(), F, st), "fusion pair " + emul)
    else:
        a_f, a_s = torch.tensor([slope], device=dev), torch.tensor([-slope], device=dev)
        fn = lib.yolat_fusion_pair_eval_f16x3_act if emul == "f16x3" else lib.yolat_fusion_pair_eval_x6_act
        check(fn(A.data_ptr(), D, N, D, *p(wf), tfold.data_ptr(), F, a_f.data_ptr(), seg.data_ptr(), seg_ptr.data_ptr(),
                 pool.data_ptr(), F, S.data_ptr(), D, P, *p(wfs), tsfold.data_ptr(), a_s.data_ptr(), Ys.data_ptr(), F, st),
              "fusion pair act " + emul)
    torch.cuda.synchronize()
    return pool.cpu(), Ys.cpu()


@pytest.mark.parametrize("slope", [None, 0.2, -0.3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("N", NS)
def test_fusion_pair_f16x3_vs_fp64_and_x6(N, F, D, layout, slope):
    c = _case(N, F, D, layout)
    P = c["P"]
    want = torch.zeros(P, F, dtype=torch.float64)
    want.index_reduce_(0, torch.from_numpy(c["seg"]).long(), _act(c["y"], slope), "amax", include_self=False)
    want_s = _act(c["ys"], None if slope is None else -slope)
    if slope is None:
        assert bool((want[:, 2] == 0).all())                     # the all-negative column pools to 0
    elif slope > 0:
        assert bool((want < 0).any()) and bool((want > 0).any())  # both signs reach the signed pooling
    else:
        assert bool((c["y"] < 0).any()) and bool((want > 0).all())  # a < 0: negative pre-activations pool as positives
    pool, Ys = _run_pair(c, slope, "f16x3")
    pool_x6, Ys_x6 = _run_pair(c, slope, "x6")
    for name, got, ref, x6 in (("pool", pool, want, pool_x6), ("super", Ys, want_s, Ys_x6)):
        scale = float(ref.abs().max())
        e64 = float((got.double() - ref).abs().max()) / scale
        ex6 = float((got - x6).abs().max()) / scale
        print("%s N=%d F=%d D=%d %s slope=%s: vs fp64 %.2e, vs x6 %.2e of the output scale" % (name, N, F, D, layout, slope,
                                                                                             e64, ex6))
        assert torch.isfinite(got).all(), name
        assert e64 <= TOL64, (name, e64)
        assert ex6 <= TOLX6, (name, ex6)
    pool2, Ys2 = _run_pair(c, slope, "f16x3")
    assert torch.equal(pool, pool2) and torch.equal(Ys, Ys2)     # deterministic


def test_fusion_pair_f16x3_wide_range_rows():
    """Operands that span ~2^26 inside every row, relu(n) * exp(3 n'): the low terms of elements more than 2^16 below their
    row's maximum are half-precision subnormals (f16x3.hpp).  Bar: 2e-6 of the output scale against float64.  The worst error
    relative to sum |a||w| is printed for both emulations (DESIGN.md 3k records it): the f16x3 error is relative to the ROW
    maxima there, not to the elements."""
    N, F, D, P = 600, 192, 128, 15
    tg = torch.Generator().manual_seed(26)
    wide = lambda *shape: torch.relu(torch.randn(*shape, generator=tg)) * torch.exp(3.0 * torch.randn(*shape, generator=tg))
    A, S, W, Ws = wide(N, D), wide(P, D), wide(F, D), wide(F, D)
    seg = (np.arange(N) // 40).astype(np.int32)
    zero, one = torch.zeros(F), torch.ones(F)
    c = dict(N=N, F=F, D=D, P=P, seg=seg, A=A, S=S, W=W, Ws=Ws, s=one, ss=one, tfold=zero, tsfold=zero)
    y = A.double() @ W.double().t()
    mag = A.double().abs() @ W.double().abs().t()
    want = torch.zeros(P, F, dtype=torch.float64)
    want.index_reduce_(0, torch.from_numpy(seg).long(), y, "amax", include_self=False)
    ys, mag_s = S.double() @ Ws.double().t(), S.double().abs() @ Ws.double().abs().t()
    for emul in ("f16x3", "x6"):
        pool, Ys = _run_pair(c, None, emul)
        e_pool = float((pool.double() - want).abs().max() / want.abs().max())
        e_sup = float((Ys.double() - ys).abs().max() / ys.abs().max())
        rel = float(((Ys.double() - ys).abs() / mag_s).max())     # per element: the super half stores every product
        print("wide range, %s: pool %.2e, super %.2e of the output scale; super worst error / sum|a||w| %.2e"
              % (emul, e_pool, e_sup, rel))
        assert e_pool <= TOL64 and e_sup <= TOL64, (emul, e_pool, e_sup)
    assert float(mag.max()) > 0


def test_fusion_pair_f16x3_keeps_subnormal_terms():
    """What f16x3.hpp states about elements far below their row's maximum: a term that is a half-precision SUBNORMAL after the
    row's scaling (here 2^-30 beside a row maximum of 1: 2^-16 scaled) still enters the product — the conversion and the MFMA
    do not flush it.  One row, two non-zero k: y[0] = 1 * 0 + 2^-30 * 1."""
    D, F = 64, 64
    A = torch.zeros(1, D)
    A[0, 0], A[0, 1] = 1.0, 2.0 ** -30
    W = torch.zeros(F, D)
    W[:, 1] = 1.0
    one, zero = torch.ones(F), torch.zeros(F)
    c = dict(N=1, F=F, D=D, P=1, seg=np.zeros(1, np.int32), A=A, S=A.clone(), W=W, Ws=W.clone(), s=one, ss=one, tfold=zero,
             tsfold=zero)
    pool, Ys = _run_pair(c, None, "f16x3")
    assert float(pool[0, 0]) == 2.0 ** -30 and float(Ys[0, 0]) == 2.0 ** -30


def test_split_f16x2_exponents_and_residual():
    """The split alone: exps[r] = 14 - floor(log2(max |row|)) (0 for a zero row, at most 127), and for every element within
    2^16 of its row's maximum ldexp(hi + lo, -exps[r]) equals the scaled weight to 2^-23 relative; zero and denormal rows
    give finite planes."""
    from yolat_vectorgraphicsrecognition_amd import ops
    rows, cols = 70, 128
    tg = torch.Generator().manual_seed(7)
    W = torch.randn(rows, cols, generator=tg) * torch.exp(3.0 * torch.randn(rows, cols, generator=tg))
    s = torch.rand(rows, generator=tg) - 0.25
    W[3] = 0.0                                                   # zero row
    W[4] = 1e-41                                                 # denormal row (after the scale too)
    s[4] = 1.0
    W[5] *= 2.0 ** 100                                           # large and tiny rows
    W[6] *= 2.0 ** -100
    hi, lo, exps = ops.split_f16x2(W.cuda(), s.cuda())
    torch.cuda.synchronize()
    hi, lo, exps = hi.cpu().double().numpy(), lo.cpu().double().numpy(), exps.cpu().numpy()
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    x = (W * s[:, None]).double().numpy()                        # fl(s W) in fp32, then exact
    mx = np.abs(x).max(1)
    want_e = np.where(mx > 0, np.minimum(14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 127), 0).astype(np.int64)
    np.testing.assert_array_equal(exps, want_e)
    assert exps[3] == 0 and exps[4] == 127 and not hi[3].any() and not lo[3].any()
    recon = np.ldexp(hi + lo, -exps[:, None].astype(np.int64))
    near = (np.abs(x) * 2.0 ** 16 >= mx[:, None]) & (x != 0)
    near[4] = False                                              # (the denormal row cannot be scaled into range)
    err = np.abs(recon - x)[near] / np.abs(x)[near]
    print("split: worst residual %.3g ulp(2^-23) over %d elements" % (err.max() * 2.0 ** 23, near.sum()))
    assert err.max() <= 2.0 ** -23
    # the scaled maximum sits in [2^14, 2^15]
    top = np.abs(hi).max(1)[mx >= 2.0 ** -112]
    assert (top >= 2.0 ** 14).all() and (top <= 2.0 ** 15).all()
