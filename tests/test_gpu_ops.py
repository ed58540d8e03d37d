"""GPU parity tests (-m gpu): every C-ABI entry point against the CPU oracle on seeded inputs.
Integer / index results must be bit-exact; fp32 features within 1e-4 relative (north_star)."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import graph_ref as gr
from oracle import oracle_np as onp
from oracle import oracle_torch as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, want, rtol=RTOL, atol=None, msg=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    scale = np.abs(want).max() if want.size else 1.0
    atol = rtol * max(scale, 1e-30) if atol is None else atol
    err = np.abs(got - want)
    bad = err > atol + rtol * np.abs(want)
    if bad.any():
        idx = np.unravel_index(np.argmax(err), err.shape)
        raise AssertionError("%s: %d/%d mismatches, max err %.3e at %s (got %.6g want %.6g), scale %.3g"
                             % (msg, bad.sum(), bad.size, err.max(), idx, got[idx], want[idx], scale))


# ---------------------------------------------------------------------------------------------
# graph pre-processing: bit-exact
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transposed", [False, True])
def test_coo_to_csr_and_csc_match_fixture(golden_dir, transposed):
    yv = _yv()
    z = np.load(os.path.join(golden_dir, "integer_ops.npz"))
    for tag in "abc":
        N = int(z["csr_%s/N" % tag])
        edge = np.stack([z["csr_%s/src" % tag], z["csr_%s/dst" % tag]], axis=1)
        E = len(edge)
        e = dev(edge)
        if transposed:
            e = e.T                                        # the model passes data.edge.T (arch:110)
        attr = torch.arange(E * 4, dtype=torch.float32).view(E, 4).cuda()
        g = yv.ops.build_graph(e, attr, None, N, 1)
        g.ensure_csc()
        g.check_status()
        for name, got in (("row_ptr", g.row_ptr), ("perm", g.perm[:E]), ("src_csr", g.src[:E]),
                          ("dst_csr", g.dst[:E]), ("col_ptr", g.col_ptr), ("slots", g.slots[:E])):
            np.testing.assert_array_equal(got.cpu().numpy(), z["csr_%s/%s" % (tag, name)],
                                          err_msg="%s %s" % (tag, name))
        np.testing.assert_array_equal(g.attr[:E].cpu().numpy(), attr.cpu().numpy()[z["csr_%s/perm" % tag]])


@pytest.mark.parametrize("N,E", [(20000, 90001), (20000, 140001), (70000, 100000), (300, 20000), (4097, 4096),
                                 (45000, 98000), (1, 7), (33, 1)])
def test_csr_large_random_matches_numpy_and_properties(N, E):
    """Both forms of yolat_graph_prepare (graph.hip) against numpy's stable argsort: the ONE-launch form for small graphs
    (k_prep_small: E <= 98304 and at most 256 rows per workgroup — every workgroup walks the whole edge list for its own
    destination rows, no exchange between workgroups) and the four-launch form above that (count / scan / fill /
    rank-and-emit).  (300, 20000) and the skewed (20000, 90001): workgroups whose rows hold more than 4096 edges take the
    kernel's ORDERED path (two more walks, stable rank from per-wave counters + lane masks); one row holds 3000 edges.
    (1, 7): one node, every edge a self loop; (33, 1): a single edge."""
    yv = _yv()
    rng = np.random.default_rng(5)
    src = rng.integers(0, N, size=E).astype(np.int64)
    dst = (rng.integers(0, N, size=E) ** 2 // N).astype(np.int64)        # skewed in-degrees
    if N == 300:
        dst[rng.permutation(E)[:3000]] = 17
    attr = torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32)).cuda()
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), attr, None, N, 1)
    g.ensure_csc()
    g.check_status()
    order = np.argsort(dst, kind="stable")
    np.testing.assert_array_equal(g.attr[:E].cpu().numpy(), attr.cpu().numpy()[order])
    np.testing.assert_array_equal(g.perm.cpu().numpy(), order.astype(np.int32))
    np.testing.assert_array_equal(g.dst.cpu().numpy(), dst[order].astype(np.int32))
    np.testing.assert_array_equal(g.src.cpu().numpy(), src[order].astype(np.int32))
    rp = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int32)
    np.testing.assert_array_equal(g.row_ptr.cpu().numpy(), rp)
    src_csr = src[order]
    order2 = np.argsort(src_csr, kind="stable")
    np.testing.assert_array_equal(g.slots.cpu().numpy(), order2.astype(np.int32))


@pytest.mark.parametrize("mix", ["grouped", "mixed", "window_edge"])
def test_csr_large_grouped_edge_list_windowed_count(mix):
    """The four-launch form on edge lists GROUPED by proposal, the order graph_dict3.py:582-600 + collate produce: the
    counting launch (k_prep_count_win) ranks a workgroup's 2048 edges in an LDS window of destination rows and sends one
    returning global atomic per touched row; a workgroup whose edges span more than 4096 rows takes the per-edge path.
    'mixed': a third of the list shuffled, so both paths run in one launch and meet in the same counters;
    'window_edge': spans of exactly 4096 and 4097 rows.  Bit-exact against numpy's stable argsort + the segment pointers."""
    yv = _yv()
    rng = np.random.default_rng(11)
    P, n_p, e_p = 2400, 25, 110
    N, E = P * n_p, P * e_p
    owner = np.repeat(np.arange(P), e_p)
    dst = owner * n_p + rng.integers(0, n_p, size=E)
    src = owner * n_p + rng.integers(0, n_p, size=E)
    if mix == "mixed":
        k = E // 3
        sel = rng.permutation(E)[:k]
        dst[sel] = rng.integers(0, N, size=k)
    if mix == "window_edge":
        dst[0], dst[1] = 0, 4095                       # workgroup 0: span 4096 (window path)
        dst[2048], dst[2049] = 100, 100 + 4096         # workgroup 1: span 4097 (per-edge path)
    bbox = np.repeat(np.arange(P), n_p).astype(np.int64)
    attr = torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32)).cuda()
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1).astype(np.int64)), attr, dev(bbox), N, P)
    g.check_status()
    order = np.argsort(dst, kind="stable")
    np.testing.assert_array_equal(g.perm.cpu().numpy(), order.astype(np.int32))
    np.testing.assert_array_equal(g.dst.cpu().numpy(), dst[order].astype(np.int32))
    np.testing.assert_array_equal(g.src.cpu().numpy(), src[order].astype(np.int32))
    np.testing.assert_array_equal(g.attr[:E].cpu().numpy(), attr.cpu().numpy()[order])
    rp = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int32)
    np.testing.assert_array_equal(g.row_ptr.cpu().numpy(), rp)
    np.testing.assert_array_equal(g.seg_ptr.cpu().numpy(), (np.arange(P + 1) * n_p).astype(np.int32))
    np.testing.assert_array_equal(g.node_seg.cpu().numpy(), bbox.astype(np.int32))


def test_graph_prepare_four_launch_form_on_small_graphs():
    """YOLAT_PREP_SMALL=0 (graph.hip, read once per process): the four-launch form of yolat_graph_prepare at the sizes
    where the one-launch kernel is the default — the integer tests of this file again in a child process."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_ops.py"), "-m", "gpu", "-q", "-x",
                        "-k", "(csr or segment_ptr or edge_range) and not four_launch"],
                       env=dict(os.environ, YOLAT_PREP_SMALL="0"), cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_edge_range_violation_is_flagged():
    yv = _yv()
    edge = dev(np.array([[0, 1], [2, 7]], dtype=np.int64))
    g = yv.ops.build_graph(edge, torch.zeros(2, 4).cuda(), None, 5, 1)
    with pytest.raises(IndexError):
        g.check_status()


def test_segment_ptr_fixture_and_unsorted_flag(golden_dir):
    yv = _yv()
    z = np.load(os.path.join(golden_dir, "integer_ops.npz"))
    bb, P = z["seg/bbox_idx"], int(z["seg/P"])
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(), dev(bb),
                           len(bb), P)
    g.check_status()
    np.testing.assert_array_equal(g.seg_ptr.cpu().numpy(), z["seg/seg_ptr"])
    np.testing.assert_array_equal(g.node_seg.cpu().numpy(), bb.astype(np.int32))
    bad = bb.copy()
    bad[3], bad[20] = bad[20], bad[3]
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(), dev(bad),
                           len(bad), P)
    with pytest.raises(ValueError):
        g.check_status()


# ---------------------------------------------------------------------------------------------
# dense layers
# ---------------------------------------------------------------------------------------------

LIN_SHAPES = [(1, 5, 64), (37, 5, 64), (64, 64, 64), (200, 14, 64), (301, 132, 64), (130, 128, 1024),
              (700, 128, 1024), (45, 2304, 512), (45, 512, 256), (45, 256, 17), (45, 256, 22), (1000, 64, 64)]


@pytest.mark.parametrize("M,K,N", LIN_SHAPES)
def test_linear_fwd_plain(M, K, N):
    yv = _yv()
    g = torch.Generator().manual_seed(M * 7 + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    Y = torch.full((M, N), float("nan")).cuda()
    yv.ops.linear_fwd(A.cuda(), W.cuda(), b.cuda(), Y)
    close(Y, A.double() @ W.double().T + b.double(), msg="linear %s" % ((M, K, N),))


def test_linear_fwd_prologue_epilogue_accumulate_and_strides():
    yv = _yv()
    g = torch.Generator().manual_seed(3)
    M, K, N = 333, 64, 64
    buf = torch.randn(M, 200, generator=g)
    A = buf[:, 40:40 + K]                                   # column slice of a wider buffer (ld=200)
    W = torch.randn(N, K, generator=g) / 8
    b = torch.randn(N, generator=g)
    asc, ash = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    osc, osh = torch.rand(N, generator=g) - 0.5, torch.randn(N, generator=g)
    ybuf = torch.randn(M, 128, generator=g)
    Yd = ybuf.cuda()
    Y = Yd[:, 64:128]
    yv.ops.linear_fwd(buf.cuda()[:, 40:40 + K], W.cuda(), b.cuda(), Y, a_pro=(asc.cuda(), ash.cuda()), a_relu=True,
                      o_pro=(osc.cuda(), osh.cuda()), o_relu=True, accumulate=True)
    a2 = torch.relu(A.double() * asc.double() + ash.double())
    want = torch.relu((a2 @ W.double().T + b.double()) * osc.double() + osh.double()) + ybuf[:, 64:128].double()
    close(Y, want, msg="pro/epi/acc")
    np.testing.assert_array_equal(Yd[:, :64].cpu().numpy(), ybuf[:, :64].numpy())   # untouched columns


@pytest.mark.parametrize("M,C,K", [(64, 64, 14), (65, 64, 64), (1000, 64, 132), (4097, 64, 64), (300, 1024, 128),
                                   (45, 512, 2304), (7, 256, 512)])
def test_linear_stats_and_bn_finalize(M, C, K):
    yv = _yv()
    g = torch.Generator().manual_seed(M + C)
    A = torch.randn(M, K, generator=g) + 0.3
    lin = torch.nn.Linear(K, C)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref_bn = torch.nn.BatchNorm1d(C)
    ref_bn.load_state_dict(bn.state_dict())
    ref_bn.train()
    with torch.no_grad():
        y = lin(A)
        z = ref_bn(y)
    lin_d, bn_d = lin.cuda(), bn.cuda()
    Y = torch.empty(M, C).cuda()
    stats = yv.ops.stats_buffer(M, C, "cuda")
    yv.ops.linear_fwd(A.cuda(), lin_d.weight, lin_d.bias, Y, stats=stats)
    coef = torch.empty(4, C).cuda()
    yv.ops.bn_finalize(stats, M, bn_d, coef[0], coef[1], coef[2], coef[3])
    close(Y, y, msg="pre-activation")
    close(coef[2], y.double().mean(0), msg="batch mean")
    close(coef[3], 1 / torch.sqrt(y.double().var(0, unbiased=False) + 1e-5), msg="invstd")
    Z = torch.empty(M, C).cuda()
    yv.ops.scale_shift_relu(Y, coef[0], coef[1], False, Z)
    close(Z, z, rtol=2e-4, msg="normalised")
    close(bn_d.running_mean, ref_bn.running_mean, msg="running_mean")
    close(bn_d.running_var, ref_bn.running_var, msg="running_var")


@pytest.mark.parametrize("M,mean,std", [(70000, 300.0, 0.02), (8000, -50.0, 1e-3), (300000, 0.0, 5.0), (33, 1e3, 0.1)])
def test_bn_finalize_offset_data(M, mean, std):
    """The BatchNorm statistics are reduced as (n, sum, sum of squares) in fp64 (dense.hip: the per-32-row partials carry M2
    about their own group mean, so only the between-group part meets the cancellation in R - S^2 / n): columns whose mean
    is up to 5e4 standard deviations away from zero must still give the batch variance to fp32 accuracy, on both reduction
    levels (M > 8192 rows) and on the single-level path."""
    yv = _yv()
    C = 64
    g = torch.Generator().manual_seed(M)
    cols = torch.linspace(0.5, 1.5, C)
    Y0 = (torch.randn(M, C, generator=g, dtype=torch.float64) * (std * cols) + mean * cols).float()
    eye = torch.eye(C).cuda()
    bn = torch.nn.BatchNorm1d(C).cuda()
    Y = torch.empty(M, C).cuda()
    stats = yv.ops.stats_buffer(M, C, "cuda")
    yv.ops.linear_fwd(Y0.cuda(), eye, None, Y, stats=stats)            # Y = Y0 exactly; the epilogue writes the partials
    assert torch.equal(Y.cpu(), Y0)
    coef = torch.empty(4, C).cuda()
    yv.ops.bn_finalize(stats, M, bn, coef[0], coef[1], coef[2], coef[3])
    yd = Y0.double()
    want_mean = yd.mean(0)
    want_var = yd.var(0, unbiased=False)
    got_var = 1.0 / coef[3].double().cpu() ** 2 - 1e-5
    assert float(((coef[2].double().cpu() - want_mean).abs() / (want_mean.abs() + want_var.sqrt())).max()) <= 2e-7
    # fp32 partials (M2 of 32 rows about their group mean) bound the accuracy, not the fp64 reduction
    assert float(((got_var - want_var).abs() / (want_var + 1e-5)).max()) <= 2e-3


def test_bn_eval_coeffs():
    yv = _yv()
    bn = torch.nn.BatchNorm1d(70)
    gu.fill_state_(bn, 9)
    x = torch.randn(33, 70)
    bn.eval()
    want = bn(x)
    bnd = torch.nn.BatchNorm1d(70)
    bnd.load_state_dict(bn.state_dict())
    bnd = bnd.cuda()
    coef = torch.empty(2, 70).cuda()
    yv.ops.bn_eval_coeffs(bnd, coef[0], coef[1])
    Z = torch.empty(33, 70).cuda()
    yv.ops.scale_shift_relu(x.cuda(), coef[0], coef[1], False, Z)
    close(Z, want, msg="bn eval")


@pytest.mark.parametrize("M,K,N", [(100, 64, 64), (777, 64, 132), (64, 1024, 128), (45, 512, 2304), (45, 17, 256),
                                   (5000, 64, 64)])
def test_linear_backward_ops(M, K, N):
    """dX = dY @ W  (linear_fwd_wt) and dW = dY^T @ A, db = colsum(dY) (linear_bwd_w); here the Linear
    is [K -> N], so W is [N, K], dY is [M, N]."""
    yv = _yv()
    g = torch.Generator().manual_seed(K + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    dY = torch.randn(M, N, generator=g)
    dX = torch.empty(M, K).cuda()
    yv.ops.linear_fwd_wt(dY.cuda(), W.cuda(), dX)
    close(dX, dY.double() @ W.double(), msg="dX")
    dW, db = torch.empty(N, K).cuda(), torch.empty(N).cuda()
    yv.ops.linear_bwd_w(dY.cuda(), A.cuda(), dW, db)
    close(dW, dY.double().T @ A.double(), msg="dW")
    close(db, dY.double().sum(0), msg="db")
    # with an A prologue (BN+ReLU of the producer) and accumulation
    sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    dW2 = dW.clone()
    yv.ops.linear_bwd_w(dY.cuda(), A.cuda(), dW2, None, a_pro=(sc.cuda(), sh.cuda()), a_relu=True, accumulate=True)
    a2 = torch.relu(A.double() * sc.double() + sh.double())
    close(dW2, dY.double().T @ a2 + dY.double().T @ A.double(), msg="dW prologue+acc")


@pytest.mark.parametrize("M,K,N", [(4100, 1896, 520), (8000, 2304, 512)])
def test_linear_bwd_w_wide_weight_takes_the_bf16x6_gemm(M, K, N):
    """dW of a wide Linear with many rows (the classifier's first layer at P = 8000) runs as transpose + pack +
    yolat_gemm_x6 (gemm_x6.hip); M not a multiple of 16 and a ragged last tile in both output dimensions; compared with the
    fp64 product at fp32-GEMM accuracy, bit-identical reruns (fixed split-K order), db from the transpose tiles."""
    yv = _yv()
    g = torch.Generator().manual_seed(M + N)
    A = torch.relu(torch.randn(M, K, generator=g))            # pooled activations are non-negative and sparse-ish
    dY = torch.randn(M, N, generator=g) * torch.rand(1, N, generator=g)
    Ad, dYd = A.cuda(), dY.cuda()
    dW, db = torch.full((N, K), 7.0).cuda(), torch.full((N,), 7.0).cuda()
    yv.ops.linear_bwd_w(dYd, Ad, dW, db)
    want = dYd.double().T @ Ad.double()
    scale = float(want.abs().max())
    assert float((dW.double() - want).abs().max()) <= 2e-6 * scale
    close(db, dYd.double().sum(0), msg="db")
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    yv.ops.linear_bwd_w(dYd, Ad, dW2, db2)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    # the accumulating form keeps the split-row fp32 kernel: same result to rounding
    dW3 = torch.zeros_like(dW)
    yv.ops.linear_bwd_w(dYd, Ad, dW3, None, accumulate=True)
    assert float((dW3.double() - want).abs().max()) <= 2e-5 * scale


@pytest.mark.parametrize("M,C,relu", [(50, 64, True), (1000, 64, True), (300, 1024, True), (45, 512, False)])
def test_bn_relu_backward(M, C, relu):
    yv = _yv()
    g = torch.Generator().manual_seed(C + M)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.2).requires_grad_(True)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    bn.train()
    z = bn(y)
    if relu:
        z = torch.relu(z)
    dz = torch.randn(M, C, generator=g)
    z.backward(dz)
    yd = y.detach().cuda()
    mean = yd.double().mean(0)
    invstd = 1 / torch.sqrt(yd.double().var(0, unbiased=False) + 1e-5)
    scale = (bn.weight.detach().cuda().double() * invstd).float()
    shift = (bn.bias.detach().cuda().double() - mean * scale.double()).float()
    dgamma, dbeta = torch.empty(C).cuda(), torch.empty(C).cuda()
    dY = torch.empty(M, C).cuda()
    yv.ops.bn_relu_bwd(dz.cuda(), yd, bn.weight.detach().cuda(), mean.float(), invstd.float(), scale, shift, relu,
                       dgamma, dbeta, dY)
    close(dY, y.grad, rtol=3e-4, msg="dY")
    close(dgamma, bn.weight.grad, rtol=3e-4, msg="dgamma")
    close(dbeta, bn.bias.grad, rtol=3e-4, msg="dbeta")


# ---------------------------------------------------------------------------------------------
# edge convolution pieces
# ---------------------------------------------------------------------------------------------

def _edge_case(N, E, Cin, seed, ldx=None):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, N, size=E).astype(np.int64)
    dst = rng.integers(0, N, size=E).astype(np.int64)
    x = rng.standard_normal((N, ldx or Cin)).astype(np.float32)
    attr = rng.standard_normal((E, 4)).astype(np.float32)
    return src, dst, x, attr


@pytest.mark.parametrize("N,E,Cin", [(10, 33, 5), (300, 1000, 5), (300, 1000, 64), (50, 0, 64), (2000, 9001, 64)])
def test_edge_lin1_forward_and_backward(N, E, Cin):
    yv = _yv()
    C = 64
    src, dst, xfull, attr = _edge_case(N, E, Cin, N + E, ldx=Cin + (64 if Cin == 64 else 0))
    x = xfull[:, :Cin]
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)) if E else torch.zeros(0, 2, dtype=torch.int64).cuda(),
                           dev(attr) if E else torch.zeros(0, 4).cuda(), None, N, 1)
    order = np.argsort(dst, kind="stable")
    tg = torch.Generator().manual_seed(1)
    W1 = torch.randn(C, 2 * Cin + 4, generator=tg) / (2 * Cin + 4) ** 0.5
    b1 = torch.randn(C, generator=tg)
    xt = torch.from_numpy(x.copy())
    s_c, d_c = torch.from_numpy(src[order]), torch.from_numpy(dst[order])
    F = torch.cat([xt[d_c], xt[s_c] - xt[d_c], torch.from_numpy(attr[order])], 1).double()
    xd = dev(xfull)[:, :Cin]
    H1 = torch.empty(max(E, 1), C).cuda()[:E]
    stats = yv.ops.stats_buffer(max(E, 1), C, "cuda")
    yv.ops.edge_lin1_fwd(xd, g, W1.cuda(), b1.cuda(), H1, stats=stats if E else None)
    if E == 0:
        return
    want = F @ W1.double().T + b1.double()
    close(H1, want, msg="H1")
    # statistics partials reduce to the batch statistics
    bn = torch.nn.BatchNorm1d(C).cuda()
    coef = torch.empty(4, C).cuda()
    yv.ops.bn_finalize(stats, E, bn, coef[0], coef[1], coef[2], coef[3])
    close(coef[2], want.mean(0), msg="edge batch mean")
    close(coef[3], 1 / torch.sqrt(want.var(0, unbiased=False) + 1e-5), msg="edge invstd")
    # weight gradient
    dH = torch.randn(E, C, generator=tg)
    dW, db = torch.empty(C, 2 * Cin + 4).cuda(), torch.empty(C).cuda()
    yv.ops.edge_lin1_bwd_w(dH.cuda(), xd, g, dW, db)
    close(dW, dH.double().T @ F, msg="dW1")
    close(db, dH.double().sum(0), msg="db1")
    # input gradient: dG then the atomic-free scatter
    dG = torch.empty(E, 2 * Cin).cuda()
    yv.ops.edge_lin1_bwd_x(dH.cuda(), W1.cuda(), Cin, dG)
    dF = dH.double() @ W1.double()
    wantG = torch.cat([dF[:, :Cin] - dF[:, Cin:2 * Cin], dF[:, Cin:2 * Cin]], 1)
    close(dG, wantG, msg="dG")
    dX = torch.randn(N, Cin).cuda()
    base = dX.clone()
    yv.ops.edge_scatter_bwd(dG, Cin, g, dX, accumulate=True)
    wantX = base.cpu().double()
    wantX.index_add_(0, d_c, wantG[:, :Cin])
    wantX.index_add_(0, s_c, wantG[:, Cin:])
    close(dX, wantX, msg="dX scatter")


@pytest.mark.parametrize("N,E,C", [(7, 20, 64), (500, 1500, 64), (100, 30, 64), (64, 640, 128)])
def test_csr_mean_forward_backward(N, E, C):
    yv = _yv()
    src, dst, _, attr = _edge_case(N, E, 4, N * 3 + E)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    order = np.argsort(dst, kind="stable")
    tg = torch.Generator().manual_seed(2)
    H = torch.randn(E, C, generator=tg)
    sc, sh = torch.rand(C, generator=tg) + 0.5, torch.randn(C, generator=tg) * 0.3
    base = torch.randn(N, C, generator=tg)
    out = base.clone().cuda()
    yv.ops.csr_mean_fwd(H.cuda(), g, out, h_pro=(sc.cuda(), sh.cuda()), h_relu=True, accumulate=True)
    m = torch.relu(H * sc + sh)
    want = orc.scatter(m, torch.from_numpy(dst[order]), dim_size=N, reduce="mean") + base
    close(out, want, msg="csr mean")
    # naive-loop oracle too (summation order = edge order)
    close(out, onp.scatter_mean(m.numpy(), dst[order], N) + base.numpy(), msg="csr mean (naive)")
    dOut = torch.randn(N, C, generator=tg)
    dM = torch.empty(E, C).cuda()
    yv.ops.csr_mean_bwd(dOut.cuda(), g, dM)
    deg = np.maximum(np.bincount(dst, minlength=N), 1)
    wantM = dOut[torch.from_numpy(dst[order])] / torch.from_numpy(deg[dst[order]]).float().view(-1, 1)
    close(dM, wantM, msg="csr mean bwd")


# ---------------------------------------------------------------------------------------------
# proposal pooling
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,D", [(13, 128), (13, 1152), (40, 1024), (3, 5)])
def test_segment_mean_max_forward_backward(P, D):
    yv = _yv()
    rng = np.random.default_rng(P * D)
    n_p = rng.integers(0, 9, size=P)
    n_p[0] = 3
    n_p[-1] = 2                                                  # last segment non-empty
    N = int(n_p.sum())
    bb = np.repeat(np.arange(P), n_p).astype(np.int64)
    X = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32))
    X[1] = X[0]                                                  # force ties inside segment 0
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(), dev(bb), N, P)
    g.check_status()
    Ym = torch.empty(P, D).cuda()
    yv.ops.segment_mean_fwd(X.cuda(), g, Ym)
    close(Ym, orc.scatter(X, torch.from_numpy(bb), dim_size=P, reduce="mean"), msg="seg mean")
    Yx = torch.empty(P, D).cuda()
    arg = torch.empty(P, D, dtype=torch.int32).cuda()
    yv.ops.segment_max_fwd(X.cuda(), g, Yx, arg)
    wx, wa = onp.scatter_max(X.numpy(), bb, P)
    np.testing.assert_array_equal(Yx.cpu().numpy(), wx)          # max is exact
    np.testing.assert_array_equal(arg.cpu().numpy(), wa.astype(np.int32))
    # prologue variant
    sc, sh = torch.rand(D) - 0.3, torch.randn(D)
    yv.ops.segment_max_fwd(X.cuda(), g, Yx, arg, x_pro=(sc.cuda(), sh.cuda()), x_relu=True)
    Xp = torch.relu(X * sc + sh)
    wx, wa = onp.scatter_max(Xp.numpy(), bb, P)
    close(Yx, wx, msg="seg max prologue")
    # backward
    dY = torch.randn(P, D)
    dX = torch.empty(N, D).cuda()
    yv.ops.segment_mean_bwd(dY.cuda(), g, dX)
    cnt = np.maximum(n_p, 1)
    close(dX, dY[torch.from_numpy(bb)] / torch.from_numpy(cnt[bb]).float().view(-1, 1), msg="seg mean bwd")
    yv.ops.segment_max_fwd(X.cuda(), g, Yx, arg)
    yv.ops.segment_max_bwd(dY.cuda(), arg, g, dX)
    Xr = X.clone().requires_grad_(True)
    orc.scatter(Xr, torch.from_numpy(bb), dim_size=P, reduce="max").backward(dY)
    np.testing.assert_array_equal(dX.cpu().numpy(), Xr.grad.numpy())


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("N,E,Cin", [(6, 7, 5), (70, 300, 5), (70, 300, 64), (1000, 4000, 64), (33, 0, 64),
                                     (500, 9000, 64), (2500, 3000, 5), (300, 700, 6), (9000, 30000, 64)])
def test_factorised_conv_layer_eval_matches_oracle(N, E, Cin, variant, fold):
    """One whole eval conv layer through the factorised kernels — yolat_conv_split_w1 (+ the folded form of
    ops.fold_factorised_layer), yolat_node_uv_eval (per-node products | root Linear | node branch) and
    yolat_edge_uv_mlp2_mean_eval_variant (node tiles / persistent fp32 / persistent bf16x6-emulated) — against the
    oracle's AttrRelativeEdgeConvGlobalPool2 in eval mode (torch_vertex.py:319-337); outputs land in column slots of
    wider buffers (ld = 128) like in the model."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    src, dst, xfull, attr = _edge_case(N, max(E, 1), Cin, 7 * N + E, ldx=Cin)
    src, dst, attr = src[:E], dst[:E], attr[:E]
    if E > 20:
        dst[:15] = 3                                  # one high-degree node
    if E > 200:
        dst[20:170] = N // 2                          # a node spanning three 64-edge passes
    conv = orc.AttrRelativeEdgeConvGlobalPool2(Cin, 64)
    gu.fill_state_(conv, 11)
    conv.eval()
    x = torch.from_numpy(xfull.copy())
    xn = torch.relu(torch.from_numpy(np.random.default_rng(1).standard_normal((N, Cin)).astype(np.float32)))
    ei = torch.from_numpy(np.stack([src, dst], 0)) if E else torch.zeros(2, 0, dtype=torch.long)
    with torch.no_grad():
        want_f, want_s = conv(x, xn, ei, None, torch.from_numpy(attr) if E else torch.zeros(0, 4))
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)) if E else torch.zeros(0, 2, dtype=torch.int64).cuda(),
                           dev(attr) if E else torch.zeros(0, 4).cuda(), None, N, 1)
    cd = conv.cuda()

    def folded(bn):
        c = torch.empty(2, 64).cuda()
        yv.ops.bn_eval_coeffs(bn, c[0], c[1])
        return c[0], c[1]

    p1, p2, pn = folded(cd.nn[1]), folded(cd.nn[4]), folded(cd.mlp_node[1])
    st = torch.cuda.current_stream().cuda_stream
    wuv, wc4 = torch.empty(128, Cin).cuda(), torch.empty(64, 4).cuda()
    check(lib.yolat_conv_split_w1(cd.nn[0].weight.data_ptr(), Cin, 64, wuv.data_ptr(), wc4.data_ptr(), st))
    uvb = None
    b1, b2 = cd.nn[0].bias, cd.nn[3].bias
    if fold:
        wuv, uvb, wc4, t2f = yv.ops.fold_factorised_layer(wuv, wc4, b1, p1[0], p1[1], b2, p2[0], p2[1])
        b1, p1, b2, p2 = None, None, None, (p2[0], t2f)
    fbuf = torch.full((N, 128), float("nan")).cuda()
    sbuf = torch.full((N, 128), float("nan")).cuda()
    UV = torch.empty(N, 128).cuda()
    xd, xnd = x.cuda(), xn.cuda()
    check(lib.yolat_node_uv_eval(xd.data_ptr(), Cin, xnd.data_ptr(), Cin, N, Cin, wuv.data_ptr(),
                                 uvb.data_ptr() if uvb is not None else None, cd.lin_r.weight.data_ptr(),
                                 cd.lin_r.bias.data_ptr(), cd.mlp_node[0].weight.data_ptr(),
                                 cd.mlp_node[0].bias.data_ptr(), pn[0].data_ptr(), pn[1].data_ptr(), 64, UV.data_ptr(), 128,
                                 fbuf[:, 64:].data_ptr(), 128, sbuf[:, :64].data_ptr(), 128, st))
    if E >= 64 or variant == 1 or E == 0:
        yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, cd.nn[3].weight, b2, p2, fbuf[:, 64:], variant=variant)
    else:
        # the persistent variants need at least one full pass; the automatic choice never picks them there
        with pytest.raises(RuntimeError):
            yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, cd.nn[3].weight, b2, p2, fbuf[:, 64:], variant=variant)
        yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, cd.nn[3].weight, b2, p2, fbuf[:, 64:], variant=0)
    close(fbuf[:, 64:], want_f, msg="factorised conv out")
    close(sbuf[:, :64], want_s, msg="factorised conv node branch")
    assert torch.isnan(fbuf[:, :64]).all() and torch.isnan(sbuf[:, 64:]).all()


@pytest.mark.parametrize("N,E,Cin", [(6, 7, 5), (70, 300, 5), (70, 300, 64), (1000, 4000, 64), (500, 9001, 64),
                                     (300, 700, 6), (2000, 33, 32), (9000, 30000, 64)])
def test_edge_mlp2_eval_is_bit_identical_to_two_kernel_path(N, E, Cin):
    """yolat_edge_mlp2_eval (both edge-MLP layers in one kernel, hidden activation in LDS) must reproduce
    yolat_edge_lin1_fwd + yolat_linear_fwd bit for bit (same k order, same epilogue arithmetic)."""
    yv = _yv()
    src, dst, xfull, attr = _edge_case(N, E, Cin, 3 * N + E, ldx=Cin)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    tg = torch.Generator().manual_seed(N + E)
    K1 = 2 * Cin + 4
    W1 = (torch.randn(64, K1, generator=tg) / K1 ** 0.5).cuda()
    W2 = (torch.randn(64, 64, generator=tg) / 8).cuda()
    b1, b2 = (torch.randn(64, generator=tg) * 0.1).cuda(), (torch.randn(64, generator=tg) * 0.1).cuda()
    p1 = ((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
    p2 = ((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
    x = dev(xfull)
    H1 = torch.empty(E, 64).cuda()
    H2a = torch.empty(E, 64).cuda()
    yv.ops.edge_lin1_fwd(x, g, W1, b1, H1, o_pro=p1, o_relu=True)
    yv.ops.linear_fwd(H1, W2, b2, H2a, o_pro=p2, o_relu=True)
    H2b = torch.full((E, 96), float("nan")).cuda()
    yv.ops.edge_mlp2_eval(x, g, W1, b1, p1, W2, b2, p2, H2b[:, :64])
    assert torch.equal(H2a, H2b[:, :64])
    assert torch.isnan(H2b[:, 64:]).all()


@pytest.mark.parametrize("N,E,Cin", [(6, 7, 5), (70, 300, 64), (1000, 4000, 64), (130, 0, 64), (2500, 3000, 5),
                                     (64, 3000, 64), (9000, 30000, 64)])
def test_node_side_eval_is_bit_identical_to_three_kernel_path(N, E, Cin):
    """yolat_node_side_eval (root Linear with the CSR mean fused into its epilogue + node-branch
    Linear+BN+ReLU, one launch) against yolat_linear_fwd + yolat_csr_mean_fwd(accumulate) + yolat_linear_fwd."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    src, dst, xfull, attr = _edge_case(N, max(E, 1), Cin, 5 * N + E, ldx=Cin)
    src, dst, attr = src[:E], dst[:E], attr[:E]
    if E > 40:
        dst[:23] = N // 2                             # a node with more than 4 in-edges (tail loop)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)) if E else torch.zeros(0, 2, dtype=torch.int64).cuda(),
                           dev(attr) if E else torch.zeros(0, 4).cuda(), None, N, 1)
    tg = torch.Generator().manual_seed(N + E + 1)
    Wr = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    Wn = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    br, bn = (torch.randn(64, generator=tg) * 0.1).cuda(), (torch.randn(64, generator=tg) * 0.1).cuda()
    pn = ((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
    f_in = dev(xfull)
    s_in = torch.randn(N, Cin, generator=tg).cuda()
    H2 = torch.randn(max(E, 1), 64, generator=tg).cuda()
    fa, sa = torch.empty(N, 64).cuda(), torch.empty(N, 64).cuda()
    yv.ops.linear_fwd(f_in, Wr, br, fa)
    if E:
        yv.ops.csr_mean_fwd(H2, g, fa, accumulate=True)
    yv.ops.linear_fwd(s_in, Wn, bn, sa, o_pro=pn, o_relu=True)
    fb = torch.full((N, 128), float("nan")).cuda()
    sb = torch.full((N, 128), float("nan")).cuda()
    st = torch.cuda.current_stream().cuda_stream
    check(lib.yolat_node_side_eval(f_in.data_ptr(), Cin, s_in.data_ptr(), Cin, N, Cin, Wr.data_ptr(), br.data_ptr(),
                                   Wn.data_ptr(), bn.data_ptr(), pn[0].data_ptr(), pn[1].data_ptr(),
                                   H2.data_ptr() if E else None, 64, g.row_ptr.data_ptr(), E, 64,
                                   fb[:, 64:].data_ptr(), 128, sb[:, :64].data_ptr(), 128, st))
    assert torch.equal(fa, fb[:, 64:]) and torch.equal(sa, sb[:, :64])
    assert torch.isnan(fb[:, :64]).all() and torch.isnan(sb[:, 64:]).all()


def test_fused_linear_segmax_and_pool_prepare_match_unfused():
    """Eval-plan kernels: fusion GEMM + BN + ReLU + per-proposal max in one launch, and the pooling
    prologue, against the oracle's scatter on the materialised activations."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    rng = np.random.default_rng(3)
    P, D, F = 37, 128, 1024
    n_p = rng.integers(1, 40, size=P)
    n_p[5] = 0                                   # an empty proposal -> zeros
    N = int(n_p.sum())
    bb = np.repeat(np.arange(P), n_p).astype(np.int64)
    tg = torch.Generator().manual_seed(4)
    feats = torch.randn(N, D, generator=tg)
    fsup = torch.randn(N, D, generator=tg)
    W = torch.randn(F, D, generator=tg) / D ** 0.5
    b = torch.randn(F, generator=tg) * 0.1
    sc, sh = torch.rand(F, generator=tg) - 0.3, torch.randn(F, generator=tg) * 0.2
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(), dev(bb), N, P)
    ZW = 2 * (F + D)
    Z = torch.full((P, ZW), float("nan")).cuda()
    st = torch.cuda.current_stream().cuda_stream
    fd, sd = feats.cuda(), fsup.cuda()
    check(lib.yolat_pool_prepare(fd.data_ptr(), sd.data_ptr(), D, D, F, g.seg_ptr.data_ptr(), P, Z.data_ptr(), ZW, st))
    Wd, bd, scd, shd = W.cuda(), b.cuda(), sc.cuda(), sh.cuda()
    check(lib.yolat_linear_segmax_fwd(fd.data_ptr(), D, N, D, Wd.data_ptr(), D, bd.data_ptr(), F, scd.data_ptr(),
                                      shd.data_ptr(), g.node_seg.data_ptr(), Z.data_ptr(), ZW, st))
    act = torch.relu((feats.double() @ W.double().T + b.double()) * sc.double() + sh.double())
    idx = torch.from_numpy(bb)
    close(Z[:, :F], orc.scatter(act.float(), idx, dim_size=P, reduce="max"), msg="fused max")
    np.testing.assert_array_equal(Z[:, F:F + D].cpu().numpy(),
                                  orc.scatter(feats, idx, dim_size=P, reduce="max").numpy())
    close(Z[:, 2 * F + D:], orc.scatter(fsup, idx, dim_size=P, reduce="mean"), msg="mean(fsup)")
    assert torch.isnan(Z[:, F + D:2 * F + D]).all()       # untouched slot (fusion_super writes it later)
    assert float(Z[5, :F].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# loss / optimiser
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,K", [(1, 17), (40, 17), (3000, 22)])
def test_softmax_ce(P, K):
    yv = _yv()
    g = torch.Generator().manual_seed(P)
    z = (torch.randn(P, K, generator=g) * 3).requires_grad_(True)
    y = torch.randint(0, K, (P,), generator=g)
    want = torch.nn.functional.cross_entropy(z, y)
    want.backward()
    loss = torch.empty(1).cuda()
    dl = torch.empty(P, K).cuda()
    yv.ops.softmax_ce(z.detach().cuda(), y.cuda(), loss, dl)
    close(loss, want.detach().reshape(1), msg="loss")
    close(dl, z.grad, msg="dlogits")


def test_adam_matches_torch_over_several_steps():
    yv = _yv()
    g = torch.Generator().manual_seed(0)
    n = 100003
    p0 = torch.randn(n, generator=g)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=2.5e-4, weight_decay=1e-5)
    pd, m, v = p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * (0.1 if step % 2 else 10.0)
        p.grad = grad.clone()
        opt.step()
        yv.ops.adam_step(pd, grad.cuda(), m, v, 2.5e-4, 0.9, 0.999, 1e-8, 1e-5, step)
    close(pd, p.detach(), rtol=1e-6, atol=1e-7, msg="adam params")
    close(m, opt.state[p]["exp_avg"], rtol=1e-5, msg="exp_avg")
    close(v, opt.state[p]["exp_avg_sq"], rtol=1e-5, msg="exp_avg_sq")


@pytest.mark.parametrize("N_P", [(37, 9), (700, 41), (5000, 300)])
def test_fusion_pool_train_matches_autograd_of_materialised_path(N_P):
    """csrc/fusion_train.hip (Gram-matrix BatchNorm statistics, extreme-of-z GEMM epilogue, sparse
    backward) against torch autograd of Linear -> BatchNorm1d(train) -> ReLU -> scatter-max in float64."""
    yv = _yv()
    Nn, P = N_P
    rng = np.random.default_rng(Nn)
    K, F = 128, 1024
    n_p = rng.multinomial(Nn - P + 1, np.ones(P - 1) / (P - 1)) + 1
    n_p = np.concatenate([n_p[:3], [0], n_p[3:]])            # one empty proposal
    n_p[-1] += Nn - n_p.sum()
    bb = np.repeat(np.arange(P), n_p).astype(np.int64)
    tg = torch.Generator().manual_seed(Nn)
    A = torch.relu(torch.randn(Nn, K, generator=tg)) + 0.3 * torch.rand(1, K, generator=tg)
    lin = torch.nn.Linear(K, F)
    bn = torch.nn.BatchNorm1d(F)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(F, K, generator=tg) / K ** 0.5)
        lin.bias.copy_(torch.randn(F, generator=tg) * 0.1)
        bn.weight.copy_(torch.rand(F, generator=tg) * 1.5 - 0.4)      # some negative gammas
        bn.bias.copy_(torch.randn(F, generator=tg) * 0.2)
    gZ = torch.randn(P, F, generator=tg) / P
    d_in = torch.randn(Nn, K, generator=tg) * 0.01                  # dA is accumulated into
    # float64 reference
    lin64, bn64 = torch.nn.Linear(K, F).double(), torch.nn.BatchNorm1d(F).double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    bn64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bn.state_dict().items()})
    A64 = A.double().requires_grad_(True)
    y = torch.relu(bn64(lin64(A64)))
    pooled = orc.scatter(y, torch.from_numpy(bb), dim=0, dim_size=P, reduce="max")
    # arg-max routing is discontinuous: where the two largest activations of a (proposal, column) are closer than fp32
    # GEMM rounding can resolve (1e-5 relative; the fp32-MFMA and the bf16x6-emulated GEMM both sit at ~1e-7..3e-7),
    # either row is a valid answer — take those entries out of the upstream gradient instead of hoping no near-tie
    # occurs among 300 x 1024 maxima
    with torch.no_grad():
        off = np.concatenate([[0], np.cumsum(n_p)])
        for pi in range(P):
            rows = y[off[pi]:off[pi + 1]]
            if rows.shape[0] >= 2:
                top = torch.topk(rows, 2, dim=0).values
                gZ[pi][((top[0] - top[1]) < 1e-5 * (top[0].abs() + 1e-3)) & (top[0] > 0)] = 0.0
    pooled.backward(gZ.double())
    # HIP
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(), dev(bb), Nn, P)
    lin_d, bn_d = lin.cuda(), bn.cuda()
    Zbuf = torch.full((P, F + 64), float("nan")).cuda()
    sv = yv.ops.fusion_pool_train_fwd(A.cuda(), lin_d, bn_d, g, Zbuf[:, :F])
    close(Zbuf[:, :F], pooled.detach().float(), rtol=2e-4, atol=2e-5, msg="pooled")
    assert torch.isnan(Zbuf[:, F:]).all()
    close(bn_d.running_mean, bn64.running_mean.float(), rtol=1e-4, atol=1e-6, msg="running_mean")
    close(bn_d.running_var, bn64.running_var.float(), rtol=1e-4, atol=1e-6, msg="running_var")
    dW, db = torch.empty(F, K).cuda(), torch.full((F,), float("nan")).cuda()
    dg, dbt = torch.empty(F).cuda(), torch.empty(F).cuda()
    dA = d_in.clone().cuda()
    yv.ops.fusion_pool_train_bwd(sv, g, gZ.cuda(), dW, db, dg, dbt, dA)

    def rel(got, want, name, tol=2e-4):
        want = want.float()
        err = float((got.cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-20)
        assert err < tol, (name, err)
    rel(dW, lin64.weight.grad, "dW")
    rel(dg, bn64.weight.grad, "dgamma")
    rel(dbt, bn64.bias.grad, "dbeta")
    rel(dA - d_in.cuda(), A64.grad, "dA")
    assert float(db.abs().max()) == 0.0 and float(lin64.bias.grad.abs().max()) < 1e-12


def test_device_subgraph_extraction_equals_loop_oracle():
    """csrc/subgraph.hip (range expansion, o2n re-indexing, run-length bbox_idx renumbering, gathers) against
    the oracle's element-wise loops of arch:153-242 — bit-exact, including duplicate ranges (later wins)."""
    yv = _yv()
    data, slices = gu.predict_case(yv.synth_batch)
    dev_batch = {k: getattr(data, k).cuda() for k in ("x", "pos", "edge", "e_attr", "bbox_idx", "bbox", "stat_feats")}
    rng = np.random.default_rng(5)
    n_roots = len(data.roots)
    for has_object in (None, rng.random(n_roots) < 0.5, np.ones(n_roots, bool)):
        ps, pe, es, ee, sb, img = yv.data.select_tree_ranges(data, slices, has_object)
        osp, ose, osb, oimg = orc.predict_gather(data, slices, None if has_object is None else torch.from_numpy(has_object))
        assert sb == osb and img == oimg
        if len(osp) == 0:
            continue
        got, status = yv.ops.extract_subgraph(yv.Data, dev_batch, ps, pe, es, ee, sb)
        want = orc.predict_build_data(data, osp, ose, osb)
        assert int(status.item()) == 0
        for k in ("x", "pos", "edge", "e_attr", "bbox", "stat_feats", "bbox_idx"):
            a, b = getattr(got, k).cpu(), getattr(want, k)
            assert a.dtype == b.dtype and torch.equal(a, b), k
    # a duplicated range: the later copy wins in the o2n table (dict semantics of the reference)
    ps, pe, es, ee, sb, _ = yv.data.select_tree_ranges(data, slices)
    ps2, pe2 = np.concatenate([ps, ps[:1]]), np.concatenate([pe, pe[:1]])
    got, status = yv.ops.extract_subgraph(yv.Data, dev_batch, ps2, pe2, es, ee, sb)
    osp = yv.data._expand_ranges(ps2, pe2).tolist()
    want = orc.predict_build_data(data, osp, yv.data._expand_ranges(es, ee).tolist(), sb)
    assert torch.equal(got.edge.cpu(), want.edge) and torch.equal(got.bbox_idx.cpu(), want.bbox_idx)
    # an edge leaving the subset raises the flag (the reference raises KeyError)
    bad = {k: v.clone() for k, v in dev_batch.items()}
    inside = set(yv.data._expand_ranges(ps, pe).tolist())
    outside = next(i for i in range(data.x.shape[0]) if i not in inside)
    bad["edge"][int(es[0]), 1] = outside
    _, status = yv.ops.extract_subgraph(yv.Data, bad, ps, pe, es, ee, sb)
    assert int(status.item()) & yv.ops.STATUS_EDGE_RANGE


def test_collate_to_device_equals_collate_fixup_and_golden(golden_dir):
    """data.collate_to_device (one pinned staging buffer, one H2D copy, offsets added by yolat_fixup_offsets)
    against collate + fixup_offsets on the host, and against the committed collate fixture."""
    yv = _yv()
    items = [yv.synth_graph(seed=900 + i, num_proposals=5 + 3 * i, nodes_lo=3, nodes_hi=9, with_roots=True)
             for i in range(4)]
    want, wslices = yv.collate([it for it in items])
    yv.fixup_offsets(want, wslices)
    got, gslices = yv.collate_to_device(items)
    for k in want.keys:
        a, b = want[k], got[k]
        if isinstance(a, torch.Tensor):
            assert b.dtype == a.dtype and tuple(b.shape) == tuple(a.shape), k
            assert torch.equal(a, b.cpu()), k
            assert torch.equal(wslices[k], gslices[k]), k
    assert all(got[k].is_cuda for k in ("x", "pos", "edge", "e_attr", "bbox_idx", "bbox", "stat_feats", "labels"))
    assert len(got.roots) == len(want.roots) and torch.equal(wslices["roots"], gslices["roots"])
    # all device tensors are views of ONE buffer (one H2D copy)
    base = got._device_buffer
    lo, hi = base.data_ptr(), base.data_ptr() + base.numel()
    assert all(lo <= got[k].data_ptr() < hi for k in ("x", "edge", "e_attr", "bbox_idx", "bbox"))
    # the committed fixture (naive-loop oracle of train.py:123-171,238-258)
    z = np.load(os.path.join(golden_dir, "collate.npz"))
    n_items = len({k.split("/")[0] for k in z.files if k.startswith("item")})
    its = []
    for i in range(n_items):
        d = yv.Data()
        for k in ("x", "pos", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
            d[k] = torch.from_numpy(z["item%d/%s" % (i, k)].copy())
        its.append(d)
    got, gslices = yv.collate_to_device(its)
    for k in ("x", "pos", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), z["batch/" + k], err_msg=k)
        np.testing.assert_array_equal(gslices[k].numpy(), z["slices/" + k], err_msg=k)
    # and it is a valid forward input
    model = yv.SparseCADGCN(yv.Opt()).cuda().eval()
    with torch.no_grad():
        out = model(got, gslices)[0]
    assert out.shape[0] == got.bbox.shape[0] and torch.isfinite(out).all()


@pytest.mark.parametrize("shape", [dict(n=4, num_proposals=9, nodes_lo=3, nodes_hi=9),
                                   dict(n=1, num_proposals=400, nodes_lo=25, nodes_hi=25, edges_per_proposal=100),
                                   dict(n=6, num_proposals=120, nodes_lo=4, nodes_hi=30, edge_factor=1.2)])
def test_collate_to_device_csr_mode_ships_the_prepared_graph(shape):
    """collate_to_device(csr=True) (native host pack + per-item CSR merged by offset-add): the prepared
    graph equals the device-side rebuild from the collated COO list bit for bit, and the eval forward (fp32 and bf16
    storage) and a training forward / backward on the csr batch equal those on the ordinary batch bit for bit."""
    yv = _yv()
    kw = dict(shape)
    n = kw.pop("n")
    items = [yv.synth_graph(seed=700 + i, **kw) for i in range(n)]
    plain, ps = yv.collate_to_device(items)
    csr, cs = yv.collate_to_device(items, csr=True)
    g = csr.__dict__["_yolat_graph"]
    N, P = int(plain.x.shape[0]), int(plain.bbox.shape[0])
    ref = yv.ops.build_graph(plain.edge, plain.e_attr, plain.bbox_idx, N, P)
    ref.check_status()
    assert (g.N, g.E, g.P) == (ref.N, ref.E, ref.P)
    for k in ("row_ptr", "src", "dst", "attr", "seg_ptr", "node_seg"):
        a, b = getattr(g, k), getattr(ref, k)
        m = min(a.shape[0], b.shape[0])
        assert torch.equal(a[:m], b[:m]), k
    for k in ("x", "bbox", "labels"):
        assert torch.equal(csr[k], plain[k]) and torch.equal(cs[k], ps[k]), k
    assert "edge" not in csr.keys and torch.equal(cs["edge"], ps["edge"])
    lo, hi = csr._device_buffer.data_ptr(), csr._device_buffer.data_ptr() + csr._device_buffer.numel()
    assert all(lo <= t.data_ptr() < hi for t in (csr.x, g.row_ptr, g.src, g.attr, g.node_seg))     # ONE H2D copy
    opt = yv.Opt()
    model = gu.fill_state_(yv.SparseCADGCN(opt), 3).cuda().eval()
    with torch.no_grad():
        a = model(plain, ps)[0]
        b = model(csr, cs)[0]
        model.set_eval_precision("bf16")
        a16 = model(plain, ps)[0]
        b16 = model(csr, cs)[0]
        model.set_eval_precision("fp32")
    assert torch.equal(a, b) and torch.equal(a16, b16)
    grads = []
    for batch, sl in ((plain, ps), (csr, cs)):
        m2 = gu.fill_state_(yv.SparseCADGCN(opt), 3).cuda().train()
        loss = yv.DetectionLoss(opt)(m2(batch, sl), batch)["loss"]
        loss.backward()
        grads.append((loss.detach().clone(), [p.grad.clone() for p in m2.parameters()]))
    assert torch.equal(grads[0][0], grads[1][0])
    for x, y in zip(grads[0][1], grads[1][1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("N,E,Cin", [(6, 7, 5), (70, 300, 64), (1000, 4000, 64), (2500, 3000, 5), (9000, 30000, 64)])
def test_factorised_edge_layer_matches_unfactorised(N, E, Cin):
    """W1.[x_i | x_j-x_i | attr] = (W1a-W1b).x_i + W1b.x_j + W1c.attr: the per-node products (yolat_node_uv_eval)
    + per-edge gather-add kernel (yolat_edge_uv_mlp2_eval) against yolat_edge_mlp2_eval; the node-side launch's
    root / node-branch outputs against yolat_linear_fwd."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    src, dst, xfull, attr = _edge_case(N, E, Cin, 11 * N + E, ldx=Cin)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    tg = torch.Generator().manual_seed(N * 3 + E)
    K1 = 2 * Cin + 4
    W1 = (torch.randn(64, K1, generator=tg) / K1 ** 0.5).cuda()
    W2 = (torch.randn(64, 64, generator=tg) / 8).cuda()
    Wr = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    Wn = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    b1, b2, br, bn = [(torch.randn(64, generator=tg) * 0.1).cuda() for _ in range(4)]
    p1, p2, pn = [((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
                  for _ in range(3)]
    x = dev(xfull)
    s_in = torch.randn(N, Cin, generator=tg).cuda()
    want = torch.empty(E, 64).cuda()
    yv.ops.edge_mlp2_eval(x, g, W1, b1, p1, W2, b2, p2, want)
    wuv, wc4 = torch.empty(128, Cin).cuda(), torch.empty(64, 4).cuda()
    st = torch.cuda.current_stream().cuda_stream
    check(lib.yolat_conv_split_w1(W1.data_ptr(), Cin, 64, wuv.data_ptr(), wc4.data_ptr(), st))
    assert torch.equal(wuv[:64], W1[:, :Cin] - W1[:, Cin:2 * Cin]) and torch.equal(wuv[64:], W1[:, Cin:2 * Cin])
    assert torch.equal(wc4, W1[:, 2 * Cin:])
    UV = torch.empty(N, 128).cuda()
    f_out, s_out = torch.empty(N, 64).cuda(), torch.empty(N, 64).cuda()
    check(lib.yolat_node_uv_eval(x.data_ptr(), Cin, s_in.data_ptr(), Cin, N, Cin, wuv.data_ptr(), None, Wr.data_ptr(),
                                 br.data_ptr(), Wn.data_ptr(), bn.data_ptr(), pn[0].data_ptr(), pn[1].data_ptr(), 64,
                                 UV.data_ptr(), 128, f_out.data_ptr(), 64, s_out.data_ptr(), 64, st))
    fa, sa = torch.empty(N, 64).cuda(), torch.empty(N, 64).cuda()
    yv.ops.linear_fwd(x, Wr, br, fa)
    yv.ops.linear_fwd(s_in, Wn, bn, sa, o_pro=pn, o_relu=True)
    assert torch.equal(fa, f_out) and torch.equal(sa, s_out)
    got = torch.full((E, 96), float("nan")).cuda()
    check(lib.yolat_edge_uv_mlp2_eval(UV.data_ptr(), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(), E,
                                      wc4.data_ptr(), b1.data_ptr(), p1[0].data_ptr(), p1[1].data_ptr(), W2.data_ptr(),
                                      b2.data_ptr(), p2[0].data_ptr(), p2[1].data_ptr(), 64, got.data_ptr(), 96, st))
    close(got[:, :64], want, rtol=2e-5, msg="factorised edge MLP")
    assert torch.isnan(got[:, 64:]).all()


@pytest.mark.parametrize("N,Cin,ldx", [(32768, 5, 5), (50001, 5, 8), (40007, 8, 8), (33000, 3, 3)])
def test_node_uv_eval_first_layer_stream_kernel(N, Cin, ldx):
    """yolat_node_uv_eval with K = in_channels <= 8 on a large graph (N >= 32768) takes the output-stream kernel
    (dense.hip k_node3_smallk: one wave per row, lane = 4 output columns): UV = x.Wuv^T + uv_bias, root = x.Wr^T + br, node
    branch = relu((s.Wn^T + bn)*sn + tn), against fp64 and — at one row below the threshold — against the MFMA tiles."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    tg = torch.Generator().manual_seed(N + Cin)
    xb = torch.randn(N, ldx, generator=tg).cuda()
    sb = torch.randn(N, ldx, generator=tg).cuda()
    x, s_in = xb[:, :Cin], sb[:, :Cin]
    wuv = (torch.randn(128, Cin, generator=tg) / Cin ** 0.5).cuda()
    Wr = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    Wn = (torch.randn(64, Cin, generator=tg) / Cin ** 0.5).cuda()
    uvb, br, bn = [(torch.randn(n, generator=tg) * 0.3).cuda() for n in (128, 64, 64)]
    sn, tn = (torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def run(n):
        UV = torch.full((n, 128), float("nan")).cuda()
        big = torch.full((n, 192), float("nan")).cuda()            # root and node branch as column slices (ld 192)
        f_out, s_out = big[:, :64], big[:, 64:128]
        check(lib.yolat_node_uv_eval(x.data_ptr(), ldx, s_in.data_ptr(), ldx, n, Cin, wuv.data_ptr(), uvb.data_ptr(),
                                     Wr.data_ptr(), br.data_ptr(), Wn.data_ptr(), bn.data_ptr(), sn.data_ptr(),
                                     tn.data_ptr(), 64, UV.data_ptr(), 128, f_out.data_ptr(), 192, s_out.data_ptr(), 192, st))
        return UV, f_out, s_out, big
    UV, f_out, s_out, big = run(N)
    xd, sd = x.double(), s_in.double()
    close(UV, xd @ wuv.double().T + uvb.double(), msg="UV")
    close(f_out, xd @ Wr.double().T + br.double(), msg="root")
    close(s_out, torch.relu((sd @ Wn.double().T + bn.double()) * sn.double() + tn.double()), msg="node branch")
    assert torch.isnan(big[:, 128:]).all()                          # nothing written past the two slices
    # the MFMA tiles on the first 32767 rows (below the threshold): same values up to the summation order
    UV2, f2, s2, _ = run(32767)
    for a_, b_ in ((UV, UV2), (f_out, f2), (s_out, s2)):
        assert float((a_[:32767] - b_).abs().max()) <= 2e-6 * float(b_.abs().max())


@pytest.mark.parametrize("N,E", [(6, 7), (70, 300), (1000, 4000), (500, 9001), (2500, 3000), (9000, 54000),
                                 (40000, 9000), (30000, 140000)])
def test_fused_edge_mean_is_bit_identical_to_edge_kernel_plus_csr_mean(N, E):
    """yolat_edge_uv_mlp2_mean_eval (node-tiled: edge MLP + mean aggregation, no [E,64] tensor) against
    yolat_edge_uv_mlp2_eval + yolat_csr_mean_fwd(accumulate); one node gets > 64 in-edges (multi-pass)."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    src, dst, _, attr = _edge_case(N, E, 64, 13 * N + E, ldx=64)
    if E > 200:
        dst[:150] = N // 3                            # a node spanning three 64-edge passes
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    tg = torch.Generator().manual_seed(N + 7 * E)
    UV = torch.randn(N, 128, generator=tg).cuda()
    W2 = (torch.randn(64, 64, generator=tg) / 8).cuda()
    wc4 = (torch.randn(64, 4, generator=tg) * 0.3).cuda()
    b1, b2 = (torch.randn(64, generator=tg) * 0.1).cuda(), (torch.randn(64, generator=tg) * 0.1).cuda()
    p1 = ((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
    p2 = ((torch.rand(64, generator=tg) - 0.2).cuda(), (torch.randn(64, generator=tg) * 0.2).cuda())
    base = torch.randn(N, 128, generator=tg).cuda()   # f_out lives in a column slot of a wider buffer
    st = torch.cuda.current_stream().cuda_stream
    H2 = torch.empty(E, 64).cuda()
    check(lib.yolat_edge_uv_mlp2_eval(UV.data_ptr(), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(), E,
                                      wc4.data_ptr(), b1.data_ptr(), p1[0].data_ptr(), p1[1].data_ptr(), W2.data_ptr(),
                                      b2.data_ptr(), p2[0].data_ptr(), p2[1].data_ptr(), 64, H2.data_ptr(), 64, st))
    want = base.clone()
    yv.ops.csr_mean_fwd(H2, g, want[:, 64:], accumulate=True)
    got = base.clone()
    check(lib.yolat_edge_uv_mlp2_mean_eval(UV.data_ptr(), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                           g.row_ptr.data_ptr(), N, E, wc4.data_ptr(), b1.data_ptr(), p1[0].data_ptr(),
                                           p1[1].data_ptr(), W2.data_ptr(), b2.data_ptr(), p2[0].data_ptr(),
                                           p2[1].data_ptr(), 64, got[:, 64:].data_ptr(), 128, st))
    if E < 131072:
        assert torch.equal(got, want)                 # automatic choice = node tiles: bit-identical
    else:                                             # automatic choice = bf16x6-emulated persistent kernel
        assert float((got - want).abs().max()) <= 2e-6 * float((want[:, 64:] - base[:, 64:]).abs().max()) + 1e-7
    # the node tiles explicitly, and the persistent wave-specialised kernel on fp32 MFMAs: same arithmetic, same order
    for variant in (yv.ops.EDGE_TILES, yv.ops.EDGE_WS_F32):
        if variant == yv.ops.EDGE_WS_F32 and E < 64:
            continue
        got = base.clone()
        yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, W2, b2, p2, got[:, 64:], variant=variant)
        assert torch.equal(got, want), "variant %d" % variant
    if E >= 64:
        # bf16x6-emulated layer 2: exact operand splits, exact products, fp32 accumulation in a different order
        got = base.clone()
        yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, W2, b2, p2, got[:, 64:], variant=yv.ops.EDGE_WS_X6)
        agg = (want[:, 64:] - base[:, 64:]).abs().max()
        assert float((got - want).abs().max()) <= 2e-6 * float(agg) + 1e-7
        again = base.clone()
        yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, W2, b2, p2, again[:, 64:], variant=yv.ops.EDGE_WS_X6)
        assert torch.equal(got, again), "bf16x6 variant is not run-to-run deterministic"
        # folded parameterisation (b1 = s1 = t1 = b2 = None): every variant against the unfused kernels
        H2 = torch.empty(E, 64).cuda()
        check(lib.yolat_edge_uv_mlp2_eval(UV.data_ptr(), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(), E,
                                          wc4.data_ptr(), None, None, None, W2.data_ptr(), None, p2[0].data_ptr(),
                                          p2[1].data_ptr(), 64, H2.data_ptr(), 64, st))
        wantf = base.clone()
        yv.ops.csr_mean_fwd(H2, g, wantf[:, 64:], accumulate=True)
        for variant in (yv.ops.EDGE_TILES, yv.ops.EDGE_WS_F32, yv.ops.EDGE_WS_X6):
            got = base.clone()
            yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, None, None, W2, None, p2, got[:, 64:], variant=variant)
            if variant == yv.ops.EDGE_WS_X6:
                aggf = (wantf[:, 64:] - base[:, 64:]).abs().max()
                assert float((got - wantf).abs().max()) <= 2e-6 * float(aggf) + 1e-7
            else:
                assert torch.equal(got, wantf), "folded, variant %d" % variant


@pytest.mark.parametrize("N,E", [(300, 1000), (50, 31), (2000, 9001), (64, 64), (1000, 4097)])
def test_factorised_training_edge_lin1_matches_gathered_gemm(N, E):
    """training-forward form of the factorised first edge Linear (yolat_edge_uv_lin1_fwd): the pre-activation H1 and
    the BatchNorm batch statistics agree with the float64 restatement of cat[x_i, x_j - x_i, attr] @ W1^T + b1 and
    with the gathered-GEMM kernel."""
    yv = _yv()
    C = Cin = 64
    src, dst, xfull, attr = _edge_case(N, E, Cin, 3 * N + E, ldx=Cin + 64)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    order = np.argsort(dst, kind="stable")
    tg = torch.Generator().manual_seed(2)
    W1 = torch.randn(C, 2 * Cin + 4, generator=tg) / (2 * Cin + 4) ** 0.5
    b1 = torch.randn(C, generator=tg)
    xt = torch.from_numpy(xfull[:, :Cin].copy())
    s_c, d_c = torch.from_numpy(src[order]), torch.from_numpy(dst[order])
    F = torch.cat([xt[d_c], xt[s_c] - xt[d_c], torch.from_numpy(attr[order])], 1).double()
    want = F @ W1.double().T + b1.double()
    xd = dev(xfull)[:, :Cin]
    H1 = torch.empty(E, C).cuda()
    stats = yv.ops.stats_buffer(E, C, "cuda")
    yv.ops.edge_lin1_fwd_factorised(xd, g, W1.cuda(), b1.cuda(), H1, stats=stats)
    close(H1, want, msg="H1 (factorised)")
    H1g = torch.empty(E, C).cuda()
    yv.ops.edge_lin1_fwd(xd, g, W1.cuda(), b1.cuda(), H1g)
    assert float((H1 - H1g).abs().max()) <= 1e-5 * float(want.abs().max())
    bn = torch.nn.BatchNorm1d(C).cuda()
    coef = torch.empty(4, C).cuda()
    yv.ops.bn_finalize(stats, E, bn, coef[0], coef[1], coef[2], coef[3])
    close(coef[2], want.mean(0), msg="edge batch mean (factorised)")
    close(coef[3], 1 / torch.sqrt(want.var(0, unbiased=False) + 1e-5), msg="edge invstd (factorised)")


@pytest.mark.parametrize("N,E,Cin", [(300, 1000, 64), (50, 31, 64), (2000, 9001, 64), (700, 5000, 5), (4000, 30000, 64)])
def test_factorised_edge_lin1_backward_matches_gathered_gemms(N, E, Cin):
    """ops.edge_lin1_bwd_factorised (per-node sums of dH1 + N-row dense algebra, csrc/edge_ops.hip yolat_edge_uv_sums)
    against the gathered path yolat_edge_lin1_bwd_w / _bwd_x / yolat_edge_scatter_bwd and against float64 autograd of
    the reference formulation cat[x_i, x_j - x_i, attr] @ W1^T (torch_vertex.py:331,335)."""
    yv = _yv()
    src, dst, xfull, attr = _edge_case(N, E, Cin, 17 * N + E, ldx=Cin)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    tg = torch.Generator().manual_seed(N + E)
    K1 = 2 * Cin + 4
    W1 = (torch.randn(64, K1, generator=tg) / K1 ** 0.5).cuda()
    dH = torch.randn(E, 64, generator=tg).cuda()          # CSR (destination-sorted) edge order, like every [E,*] tensor
    x = dev(xfull)
    base = torch.randn(N, Cin, generator=tg).cuda()
    # gathered path
    dW_a, db_a = torch.empty(64, K1).cuda(), torch.empty(64).cuda()
    yv.ops.edge_lin1_bwd_w(dH, x, g, dW_a, db_a)
    dx_a = base.clone()
    dG = torch.empty(E, 2 * Cin).cuda()
    yv.ops.edge_lin1_bwd_x(dH, W1, Cin, dG)
    yv.ops.edge_scatter_bwd(dG, Cin, g, dx_a, accumulate=True)
    # factorised path
    dW_b, db_b = torch.empty(64, K1).cuda(), torch.empty(64).cuda()
    dx_b = base.clone()
    yv.ops.edge_lin1_bwd_factorised(dH, x, g, W1, dW_b, db_b, dx=dx_b, dx_accumulate=True)
    # float64 autograd of the reference formulation, on the CSR-ordered edge list
    xs = x.double().cpu().requires_grad_(True)
    Wd = W1.double().cpu().requires_grad_(True)
    bd = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    s, d = g.src.cpu().long()[:E], g.dst.cpu().long()[:E]
    F = torch.cat([xs[d], xs[s] - xs[d], g.attr.cpu().double()[:E]], 1)
    ((F @ Wd.t() + bd) * dH.double().cpu()).sum().backward()
    for name, got, want in (("dW1", dW_b, Wd.grad), ("db1", db_b, bd.grad), ("dx", dx_b - base, xs.grad)):
        scale = float(want.abs().max())
        assert float((got.double().cpu() - want).abs().max()) <= 2e-5 * scale, name
    for name, a, b in (("dW1", dW_a, dW_b), ("db1", db_a, db_b), ("dx", dx_a, dx_b)):
        assert float((a - b).abs().max()) <= 5e-5 * float(a.abs().max()), name
    # deterministic
    dW_c, db_c = torch.empty(64, K1).cuda(), torch.empty(64).cuda()
    dx_c = base.clone()
    yv.ops.edge_lin1_bwd_factorised(dH, x, g, W1, dW_c, db_c, dx=dx_c, dx_accumulate=True)
    assert torch.equal(dW_b, dW_c) and torch.equal(db_b, db_c) and torch.equal(dx_b, dx_c)


@pytest.mark.parametrize("N,E", [(300, 1000), (50, 31), (2000, 9001), (700, 5000), (4000, 30000), (64, 513)])
def test_fused_bn_csr_backward_matches_materialised_path(N, E):
    """ops.BnCsrGrad (bn_csr.hip: the gradient w.r.t. the second edge Linear's output formed inside the loaders of its
    consumers) against the materialising sequence csr_mean_bwd -> bn_relu_bwd -> linear_bwd_w / linear_fwd_wt, and
    against float64 autograd of mean-aggregate(relu(batchnorm(Y))) (torch_vertex.py:308,324 + torch_nn.py:58-66)."""
    yv = _yv()
    C = 64
    src, dst, xfull, attr = _edge_case(N, E, 64, 3 * N + E, ldx=64)
    g = yv.ops.build_graph(dev(np.stack([src, dst], 1)), dev(attr), None, N, 1)
    tg = torch.Generator().manual_seed(N + 7 * E)
    d_f = torch.randn(N, C, generator=tg).cuda()
    H2 = torch.randn(E, C, generator=tg).cuda()
    H1 = torch.randn(E, C, generator=tg).cuda()
    W = (torch.randn(C, C, generator=tg) / 8).cuda()
    c1 = torch.stack([torch.rand(C, generator=tg) + 0.5, torch.randn(C, generator=tg)]).cuda()     # prologue of H1
    gamma = (torch.rand(C, generator=tg) + 0.5).cuda()
    beta = torch.randn(C, generator=tg).cuda()
    mean, var = H2.mean(0), H2.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    scale = gamma * invstd
    shift = beta - mean * scale
    coefs = torch.stack([scale, shift, mean, invstd]).contiguous()
    # materialising path
    dM = torch.empty(E, C).cuda()
    yv.ops.csr_mean_bwd(d_f, g, dM)
    dg_a, db_a = torch.empty(C).cuda(), torch.empty(C).cuda()
    yv.ops.bn_relu_bwd(dM, H2, gamma, coefs[2], coefs[3], coefs[0], coefs[1], True, dg_a, db_a, dM)
    dW_a, dbias_a = torch.empty(C, C).cuda(), torch.empty(C).cuda()
    yv.ops.linear_bwd_w(dM, H1, dW_a, dbias_a, a_pro=(c1[0], c1[1]), a_relu=True)
    dA_a = torch.empty(E, C).cuda()
    yv.ops.linear_fwd_wt(dM, W, dA_a)

    def fused():
        dg, db = torch.empty(C).cuda(), torch.empty(C).cuda()
        dW, dbias, dA = torch.empty(C, C).cuda(), torch.empty(C).cuda(), torch.empty(E, C).cuda()
        h = yv.ops.BnCsrGrad(d_f, g, H2, coefs[2], coefs[3], coefs[0], coefs[1], relu=True)
        h.stats(dg, db)
        h.bwd_w(H1, dW, dbias, a_pro=(c1[0], c1[1]), a_relu=True)
        h.fwd_wt(W, dA)
        return dg, db, dW, dbias, dA
    got = fused()
    for name, a, b in zip(("dgamma", "dbeta", "dW", "db", "dA"), (dg_a, db_a, dW_a, dbias_a, dA_a), got):
        # db = column sums of dY is exactly 0 in exact arithmetic (BatchNorm's backward): both paths return rounding noise
        # of the sum, which moves with the block size of the statistics pass — measured against the column sums of |dY|
        ref_scale = float(dM.abs().sum(0).max()) if name == "db" else max(float(a.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 2e-5 * ref_scale, name

    def fused_one_kernel():
        dg, db = torch.empty(C).cuda(), torch.empty(C).cuda()
        dW, dbias, dA = torch.empty(C, C).cuda(), torch.empty(C).cuda(), torch.full((E, C), -7.0).cuda()
        h = yv.ops.BnCsrGrad(d_f, g, H2, coefs[2], coefs[3], coefs[0], coefs[1], relu=True)
        h.stats(dg, db)
        h.bwd_w_and_x(H1, W, dW, dbias, dA, a_pro=(c1[0], c1[1]), a_relu=True)
        return dg, db, dW, dbias, dA
    one = fused_one_kernel()
    for name, a, b in zip(("dgamma", "dbeta", "dW", "db", "dA"), (dg_a, db_a, dW_a, dbias_a, dA_a), one):
        ref_scale = float(dA_a.abs().sum(0).max()) if name == "db" else max(float(a.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 2e-5 * ref_scale, name
    for a, b in zip(one, fused_one_kernel()):
        assert torch.equal(a, b)
    # ... and with the statistics of the NEXT BatchNorm's backward (the one behind the prologue of A) taken in the same
    # kernel: against bn_relu_bwd on the materialised dA
    m1, is1 = H1.mean(0), 1 / torch.sqrt(H1.var(0, unbiased=False) + 1e-5)
    g1 = (torch.rand(C, generator=tg) + 0.5).cuda()
    b1 = torch.randn(C, generator=tg).cuda()
    cc1 = torch.stack([g1 * is1, b1 - m1 * g1 * is1, m1, is1]).contiguous()
    dW_r, dbias_r = torch.empty(C, C).cuda(), torch.empty(C).cuda()
    yv.ops.linear_bwd_w(dM, H1, dW_r, dbias_r, a_pro=(cc1[0], cc1[1]), a_relu=True)
    dg1_r, db1_r, dH1_r = torch.empty(C).cuda(), torch.empty(C).cuda(), torch.empty(E, C).cuda()
    yv.ops.bn_relu_bwd(dA_a, H1, g1, cc1[2], cc1[3], cc1[0], cc1[1], True, dg1_r, db1_r, dH1_r)
    h = yv.ops.BnCsrGrad(d_f, g, H2, coefs[2], coefs[3], coefs[0], coefs[1], relu=True)
    h.stats(torch.empty(C).cuda(), torch.empty(C).cuda())
    dW_n, dbias_n, dA_n = torch.empty(C, C).cuda(), torch.empty(C).cuda(), torch.empty(E, C).cuda()
    dg1_n, db1_n = torch.empty(C).cuda(), torch.empty(C).cuda()
    coef1 = h.bwd_w_and_x(H1, W, dW_n, dbias_n, dA_n, a_pro=(cc1[0], cc1[1]), a_relu=True,
                          next_bn=(cc1[2], cc1[3], dg1_n, db1_n))
    assert float((dA_n - dA_a).abs().max()) <= 2e-5 * float(dA_a.abs().max())
    assert float((dW_n - dW_r).abs().max()) <= 2e-5 * float(dW_r.abs().max())
    yv.ops.bn_relu_bwd_apply(dA_n, H1, cc1[2], cc1[3], cc1[0], cc1[1], True, coef1, dA_n)
    for name, a, b in (("dgamma1", dg1_r, dg1_n), ("dbeta1", db1_r, db1_n), ("dH1", dH1_r, dA_n)):
        assert float((a - b).abs().max()) <= 5e-5 * max(float(a.abs().max()), 1e-6), name
    again = fused()
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                             # deterministic
    # float64 autograd of the reference formulation (CSR edge order)
    Y = H2.double().cpu().requires_grad_(True)
    gam = gamma.double().cpu().requires_grad_(True)
    bet = beta.double().cpu().requires_grad_(True)
    d = g.dst.cpu().long()[:E]
    z = torch.relu(torch.nn.functional.batch_norm(Y, None, None, gam, bet, True, 0.0, 1e-5))
    deg = torch.bincount(d, minlength=N).clamp_min(1).double()
    out = torch.zeros(N, C, dtype=torch.float64).index_add_(0, d, z) / deg[:, None]
    (out * d_f.double().cpu()).sum().backward()
    dY = Y.grad
    a1 = torch.relu(H1.double().cpu() * c1[0].double().cpu() + c1[1].double().cpu())
    want = (gam.grad, bet.grad, dY.t() @ a1, dY.sum(0), dY @ W.double().cpu())
    for name, b, w in zip(("dgamma", "dbeta", "dW", "db", "dA"), got, want):
        # db = column sums of dY is exactly 0 in exact arithmetic (BatchNorm's backward): measure it against the column
        # sums of |dY|
        ref = float(dY.abs().sum(0).max()) if name == "db" else max(float(w.abs().max()), 1e-6)
        assert float((b.double().cpu() - w).abs().max()) <= 5e-5 * ref, name


@pytest.mark.parametrize("N,P,D", [(700, 30, 128), (10000, 400, 128), (257, 5, 64), (5000, 4999, 128)])
def test_fusion_x6_matches_fp32_fusion_kernel(N, P, D):
    """yolat_fusion_pair_eval_x6 (fusion GEMM emulated with six bf16 MFMA products on exactly split operands, BatchNorm
    scale folded into the weights) against yolat_fusion_pair_eval (fp32 MFMAs): pooled maxima and the super branch."""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    F = 1024
    tg = torch.Generator().manual_seed(N + P)
    A = torch.randn(N, D, generator=tg).cuda()
    S = torch.randn(P, D, generator=tg).cuda()
    Wf, Wfs = (torch.randn(F, D, generator=tg) / D ** 0.5).cuda(), (torch.randn(F, D, generator=tg) / D ** 0.5).cuda()
    bf, bfs = (torch.randn(F, generator=tg) * 0.1).cuda(), (torch.randn(F, generator=tg) * 0.1).cuda()
    sf, sfs = (torch.rand(F, generator=tg) - 0.3).cuda(), (torch.rand(F, generator=tg) + 0.5).cuda()    # some negative scales
    tf, tfs = (torch.randn(F, generator=tg) * 0.2).cuda(), (torch.randn(F, generator=tg) * 0.2).cuda()
    seg = torch.sort(torch.randint(0, P, (N,), generator=tg))[0].int().cuda()
    st = torch.cuda.current_stream().cuda_stream
    ZW = 2 * (F + D)
    Za, Zb = torch.zeros(P, ZW).cuda(), torch.zeros(P, ZW).cuda()
    check(lib.yolat_fusion_pair_eval(A.data_ptr(), D, N, D, Wf.data_ptr(), bf.data_ptr(), sf.data_ptr(), tf.data_ptr(), F,
                                     seg.data_ptr(), Za.data_ptr(), ZW, S.data_ptr(), D, P, Wfs.data_ptr(), bfs.data_ptr(),
                                     sfs.data_ptr(), tfs.data_ptr(), Za[:, F + D:].data_ptr(), ZW, st))
    parts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    check(lib.yolat_split_bf16x3(Wf.data_ptr(), D, F, D, sf.data_ptr(), parts[0].data_ptr(), parts[1].data_ptr(),
                                 parts[2].data_ptr(), st))
    scaled = (Wf * sf[:, None]).flatten()
    assert torch.equal(parts[0].float() + parts[1].float() + parts[2].float(), scaled)      # the split is exact
    tfold = sf * bf + tf
    sparts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    check(lib.yolat_split_bf16x3(Wfs.data_ptr(), D, F, D, sfs.data_ptr(), sparts[0].data_ptr(), sparts[1].data_ptr(),
                                 sparts[2].data_ptr(), st))
    tsfold = sfs * bfs + tfs

    def x6(Z):
        check(lib.yolat_fusion_pair_eval_x6(A.data_ptr(), D, N, D, parts[0].data_ptr(), parts[1].data_ptr(),
                                            parts[2].data_ptr(), tfold.data_ptr(), F, seg.data_ptr(), Z.data_ptr(), ZW,
                                            S.data_ptr(), D, P, sparts[0].data_ptr(), sparts[1].data_ptr(),
                                            sparts[2].data_ptr(), tsfold.data_ptr(), Z[:, F + D:].data_ptr(), ZW, st))

    x6(Zb)
    sup_a, sup_b = Za[:, F + D:2 * F + D], Zb[:, F + D:2 * F + D]
    assert float((sup_a - sup_b).abs().max()) <= 3e-6 * float(sup_a.abs().max())            # super branch
    scale = float(Za[:, :F].abs().max())
    assert float((Za[:, :F] - Zb[:, :F]).abs().max()) <= 3e-6 * scale
    # against float64
    want = torch.zeros(P, F, dtype=torch.float64)
    act = torch.relu((A.double().cpu() @ Wf.double().cpu().t() + bf.double().cpu()) * sf.double().cpu() + tf.double().cpu())
    want.index_reduce_(0, seg.cpu().long(), act, "amax", include_self=True)
    assert float((Zb[:, :F].double().cpu() - want).abs().max()) <= 2e-6 * scale
    Zc = torch.zeros(P, ZW).cuda()
    x6(Zc)
    assert torch.equal(Zb, Zc)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,relu", [(400, 2304, 512, 1), (400, 512, 256, 1), (400, 256, 10, 0), (1, 64, 33, 0),
                                         (8000, 2304, 512, 1), (37, 48, 70, 1)])
def test_linear_x6_matches_fp64(M, K, N, relu):
    """yolat_linear_x6 (bf16x6-emulated skinny Linear with folded BatchNorm + ReLU) against the fp64 product of the
    same operands: fp32-class accuracy (5e-6 of the output scale; the fp32 MFMA kernel sits at ~1e-6), deterministic,
    and edge sizes (one row, N not a multiple of 32, K = 48)."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    gen = torch.Generator().manual_seed(M + K + N)
    A = torch.randn(M, K, generator=gen).cuda()
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).cuda()
    s = (torch.rand(N, generator=gen) + 0.5).cuda()
    shift = torch.randn(N, generator=gen).cuda()
    st = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(lib.yolat_split_bf16x3_packed_elems(N, K), dtype=torch.bfloat16, device="cuda")
    check(lib.yolat_split_bf16x3_packed(W.data_ptr(), K, N, K, s.data_ptr(), packed.data_ptr(), st))
    # the split is exact and the packing is the documented one: [ct][ks][part][lane][8]
    pk = packed.view((N + 31) // 32, K // 16, 3, 2, 32, 8).double().sum(2)       # [ct, ks, lhi, j, e]
    rec = pk.permute(0, 3, 1, 2, 4).reshape(-1, K)[:N]                           # [ct*32 + j, ks*16 + lhi*8 + e]
    assert torch.equal(rec, (s[:, None] * W).double())
    out = torch.full((M, N + 3), -7.0, device="cuda")

    def run(o, k=K):
        return lib.yolat_linear_x6(A.data_ptr(), K, M, k, packed.data_ptr(), shift.data_ptr(), relu, N, o.data_ptr(),
                                   N + 3, st)
    check(run(out))
    ref = A.double() @ (s[:, None] * W).double().t() + shift.double()
    if relu:
        ref = ref.clamp_min(0)
    scale = float(ref.abs().max())
    assert float((out[:, :N].double() - ref).abs().max()) <= 5e-6 * scale
    assert torch.all(out[:, N:] == -7.0)                                   # nothing written past N
    out2 = torch.full((M, N + 3), -7.0, device="cuda")
    check(run(out2))
    assert torch.equal(out, out2)
    assert run(out, K - 1) != 0                                            # contract: K % 16 == 0
    # A pre-split and packed (the long-K path): same accuracy class, deterministic
    apk = torch.empty(lib.yolat_split_bf16x3_packed_elems(M, K), dtype=torch.bfloat16, device="cuda")
    check(lib.yolat_split_bf16x3_packed(A.data_ptr(), K, M, K, None, apk.data_ptr(), st))
    out3 = torch.full((M, N + 3), -7.0, device="cuda")
    check(lib.yolat_linear_x6_pre(apk.data_ptr(), M, K, packed.data_ptr(), shift.data_ptr(), relu, N, out3.data_ptr(),
                                  N + 3, st))
    assert float((out3[:, :N].double() - ref).abs().max()) <= 5e-6 * scale
    assert torch.all(out3[:, N:] == -7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,relu", [(400, 2304, 512, 1), (2000, 2304, 512, 1), (8000, 2304, 512, 1), (1, 64, 33, 0),
                                         (37, 48, 70, 1), (129, 256, 129, 0), (20000, 64, 256, 1)])
def test_gemm_x6_matches_fp64(M, K, N, relu):
    """yolat_gemm_x6 (LDS-tiled bf16x6-emulated Linear with folded BatchNorm + ReLU, split-K for few rows) against the
    fp64 product of the same operands: fp32-class accuracy (5e-6 of the output scale), deterministic, nothing written
    past N, and the edge sizes (one row, ragged M / N, K = 48, both the split-K and the direct path)."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    gen = torch.Generator().manual_seed(M + K + N)
    A = torch.randn(M, K, generator=gen).cuda()
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).cuda()
    s = (torch.rand(N, generator=gen) + 0.5).cuda()
    shift = torch.randn(N, generator=gen).cuda()
    st = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(lib.yolat_gemm_x6_packed_elems(N, K), dtype=torch.bfloat16, device="cuda")
    check(lib.yolat_gemm_x6_pack(W.data_ptr(), K, N, K, s.data_ptr(), packed.data_ptr(), st))
    work = torch.empty(max(1, lib.yolat_gemm_x6_work_elems(M, N, K)), device="cuda")
    ref = A.double() @ (s[:, None] * W).double().t() + shift.double()
    if relu:
        ref = ref.clamp_min(0)
    scale = float(ref.abs().max())
    outs = []
    for _ in range(2):
        out = torch.full((M, N + 3), -7.0, device="cuda")
        check(lib.yolat_gemm_x6(A.data_ptr(), K, M, K, packed.data_ptr(), shift.data_ptr(), relu, N, out.data_ptr(), N + 3,
                                work.data_ptr(), st))
        outs.append(out)
    assert float((outs[0][:, :N].double() - ref).abs().max()) <= 5e-6 * scale
    assert torch.all(outs[0][:, N:] == -7.0)
    assert torch.equal(outs[0], outs[1])
    assert lib.yolat_gemm_x6(A.data_ptr(), K, M, K - 1, packed.data_ptr(), None, 0, N, outs[0].data_ptr(), N + 3,
                             work.data_ptr(), st) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 255, 1000, 43520])
def test_node_uv_eval_x6_matches_fp32_node_side(N):
    """yolat_node_uv_eval_x6 (node side of a factorised conv layer on the bf16x6 rows kernel: stacked [Wuvf ; Wr] and
    the node branch with its BatchNorm scale folded into the weights) against yolat_node_uv_eval (fp32-MFMA tiles) on
    the same operands, strided outputs (concat slots), ragged N; deterministic."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    C = 64
    gen = torch.Generator().manual_seed(N)
    f_in = torch.randn(N, 2 * C, generator=gen).cuda()[:, :C]            # ld 128: a concat slot
    s_in = torch.randn(N, C, generator=gen).cuda()
    Wuv = (torch.randn(2 * C, C, generator=gen) / 8).cuda()
    uvb = torch.randn(2 * C, generator=gen).cuda()
    Wr, br = (torch.randn(C, C, generator=gen) / 8).cuda(), torch.randn(C, generator=gen).cuda()
    Wn, bn = (torch.randn(C, C, generator=gen) / 8).cuda(), torch.randn(C, generator=gen).cuda()
    sn, tn = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def outs():
        return torch.full((N, 2 * C), -7.0).cuda(), torch.full((N, 3 * C), -7.0).cuda(), torch.full((N, 3 * C), -7.0).cuda()
    UVa, fa, sa = outs()
    check(lib.yolat_node_uv_eval(f_in.data_ptr(), 2 * C, s_in.data_ptr(), C, N, C, Wuv.data_ptr(), uvb.data_ptr(),
                                 Wr.data_ptr(), br.data_ptr(), Wn.data_ptr(), bn.data_ptr(), sn.data_ptr(), tn.data_ptr(), C,
                                 UVa.data_ptr(), 2 * C, fa[:, C:].data_ptr(), 3 * C, sa[:, C:].data_ptr(), 3 * C, st))

    def split(w, scale):
        parts = [torch.empty(w.numel(), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
        check(lib.yolat_split_bf16x3(w.data_ptr(), w.shape[1], w.shape[0], w.shape[1],
                                     scale.data_ptr() if scale is not None else None, parts[0].data_ptr(),
                                     parts[1].data_ptr(), parts[2].data_ptr(), st))
        return parts
    wfr = torch.cat([Wuv, Wr], 0).contiguous()
    tfr = torch.cat([uvb, br], 0).contiguous()
    pfr, pn = split(wfr, None), split(Wn, sn)
    tnf = (sn * bn + tn).contiguous()

    def run():
        UV, f, s = outs()
        check(lib.yolat_node_uv_eval_x6(f_in.data_ptr(), 2 * C, s_in.data_ptr(), C, N, pfr[0].data_ptr(), pfr[1].data_ptr(),
                                        pfr[2].data_ptr(), tfr.data_ptr(), pn[0].data_ptr(), pn[1].data_ptr(),
                                        pn[2].data_ptr(), tnf.data_ptr(), UV.data_ptr(), 2 * C, f[:, C:].data_ptr(), 3 * C,
                                        s[:, C:].data_ptr(), 3 * C, st))
        return UV, f, s
    UVb, fb, sb = run()
    for name, a, b in (("UV", UVa, UVb), ("f_out", fa, fb), ("s_out", sa, sb)):
        assert float((a - b).abs().max()) <= 3e-6 * float(a.abs().max()), name
    assert torch.all(fb[:, :C] == -7.0) and torch.all(fb[:, 2 * C:] == -7.0)      # nothing outside the slots
    assert torch.all(sb[:, :C] == -7.0) and torch.all(sb[:, 2 * C:] == -7.0)
    for a, b in zip((UVb, fb, sb), run()):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(8000, 512, 2304), (2000, 512, 2304), (1024, 256, 512)])
def test_linear_fwd_wt_x6_path_matches_fp64(M, K, N):
    """ops.linear_fwd_wt (dX = dY . W of a Linear's backward) on the bf16x6 GEMM with the transposed pack
    (yolat_gemm_x6_pack_t) — the shapes that take that path — against the float64 product; deterministic."""
    yv = _yv()
    gen = torch.Generator().manual_seed(M + N)
    dY = torch.randn(M, K, generator=gen).cuda()
    W = (torch.randn(K, N, generator=gen) / K ** 0.5).cuda()
    outs = []
    for _ in range(2):
        dX = torch.full((M, N), -7.0).cuda()
        yv.ops.linear_fwd_wt(dY, W, dX)
        outs.append(dX)
    ref = dY.double() @ W.double()
    assert float((outs[0].double() - ref).abs().max()) <= 5e-6 * float(ref.abs().max())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(70000, 64, 64), (65536 + 17, 128, 128)])
def test_linear_fwd_rows_x6_path_matches_fp32_kernel_and_statistics(M, K, N):
    """ops.linear_fwd on the bf16x6 rows kernel (yolat_linear_fwd_rows_x6: many rows, K in {64, 128}, BatchNorm + ReLU
    prologue on A, pre-activation output + BatchNorm partial statistics) against the fp32-MFMA kernel on the same
    operands (ops.X6_TRAIN_ROWS flipped in-process; the path is opt-in: it measured equal to the fp32 tiles), and the
    finalized statistics against float64."""
    yv = _yv()
    gen = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=gen).cuda()
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).cuda()
    b = torch.randn(N, generator=gen).cuda()
    pro = ((torch.rand(K, generator=gen) + 0.5).cuda(), torch.randn(K, generator=gen).cuda())

    def run(x6):
        old = yv.ops.X6_TRAIN_ROWS
        yv.ops.X6_TRAIN_ROWS = x6
        try:
            Y = torch.full((M, N + 4), -7.0).cuda()
            st = yv.ops.stats_buffer(M, N, A.device)
            yv.ops.linear_fwd(A, W, b, Y[:, :N], a_pro=pro, a_relu=True, stats=st)
            bn = torch.nn.BatchNorm1d(N).cuda()
            coef = torch.empty(4, N).cuda()
            yv.ops.bn_finalize(st, M, bn, coef[0], coef[1], coef[2], coef[3])
            return Y, coef
        finally:
            yv.ops.X6_TRAIN_ROWS = old
    Ya, ca = run(False)
    Yb, cb = run(True)
    scale = float(Ya[:, :N].abs().max())
    assert float((Ya[:, :N] - Yb[:, :N]).abs().max()) <= 3e-6 * scale
    assert torch.all(Yb[:, N:] == -7.0)
    ref = torch.relu(A.double() * pro[0].double() + pro[1].double()) @ W.double().t() + b.double()
    close(cb[2], ref.mean(0).float(), rtol=1e-4, atol=1e-5, msg="batch mean")
    close(cb[3], (1 / torch.sqrt(ref.var(0, unbiased=False) + 1e-5)).float(), rtol=1e-4, atol=1e-6, msg="invstd")
    Yc, cc = run(True)
    assert torch.equal(Yb, Yc) and torch.equal(cb, cc)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(8000, 2304, 512), (4100, 256, 130)])
def test_linear_fwd_gemm_x6_stats_path_matches_fp32_kernel(M, K, N):
    """ops.linear_fwd with BatchNorm statistics on the bf16x6 LDS-tiled GEMM (yolat_gemm_x6_stats: the training-mode
    classifier layer at P = 8000) against the fp32-MFMA kernel (ops.X6_TRAIN_GEMM flipped in-process): outputs, and the
    finalized statistics against float64."""
    yv = _yv()
    gen = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=gen).cuda()
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).cuda()
    b = torch.randn(N, generator=gen).cuda()

    def run(x6):
        old = yv.ops.X6_TRAIN_GEMM
        yv.ops.X6_TRAIN_GEMM = x6
        try:
            Y = torch.full((M, N + 4), -7.0).cuda()
            st = yv.ops.stats_buffer(M, N, A.device)
            yv.ops.linear_fwd(A, W, b, Y[:, :N], stats=st)
            coef = torch.empty(4, N).cuda()
            yv.ops.bn_finalize(st, M, torch.nn.BatchNorm1d(N).cuda(), coef[0], coef[1], coef[2], coef[3])
            return Y, coef
        finally:
            yv.ops.X6_TRAIN_GEMM = old
    Ya, ca = run(False)
    Yb, cb = run(True)
    assert float((Ya[:, :N] - Yb[:, :N]).abs().max()) <= 5e-6 * float(Ya[:, :N].abs().max())
    assert torch.all(Yb[:, N:] == -7.0)
    ref = A.double() @ W.double().t() + b.double()
    close(cb[2], ref.mean(0).float(), rtol=1e-4, atol=1e-5, msg="batch mean")
    close(cb[3], (1 / torch.sqrt(ref.var(0, unbiased=False) + 1e-5)).float(), rtol=1e-4, atol=1e-6, msg="invstd")
    Yc, cc = run(True)
    assert torch.equal(Yb, Yc) and torch.equal(cb, cc)


@pytest.mark.parametrize("E,half", [(1, False), (63, False), (1000, True), (300001, False), (300001, True)])
def test_edge_attr_dw_streaming_reduction_matches_fp64(E, half):
    """yolat_edge_attr_dw (edge_ops.hip k_attr_dw): dWc4 = dH1^T . attr and db1 = column sums of dH1 — the part of the first edge
    Linear's weight gradient that reads the edge attributes (torch_vertex.py:331) — against fp64, for fp32 and
    bfloat16-stored gradients, ragged sizes, with and without the bias gradient; run-to-run bit identity."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    gen = torch.Generator().manual_seed(E + int(half))
    dH = torch.randn(E, 64, generator=gen)
    attr = (torch.randn(E, 4, generator=gen) * (torch.rand(E, 1, generator=gen) > 0.85)).contiguous()     # 85 % zero rows
    dHd = dH.to(torch.bfloat16).cuda() if half else dH.cuda()
    ref_w = dHd.double().cpu().t() @ attr.double()
    ref_b = dHd.double().cpu().sum(0)
    attr = attr.cuda()
    work = torch.empty(lib.yolat_edge_attr_dw_work_elems(E), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for with_b in (True, False, True):
        dw = torch.full((64, 4), float("nan"), device="cuda")
        db = torch.full((64,), float("nan"), device="cuda")
        check(lib.yolat_edge_attr_dw(dHd.data_ptr(), 64, int(half), attr.data_ptr(), E, 64, dw.data_ptr(),
                                     db.data_ptr() if with_b else None, work.data_ptr(), st))
        outs.append((dw, db))
        assert float((dw.double().cpu() - ref_w).abs().max()) <= 2e-6 * max(float(ref_w.abs().max()), 1e-3) * max(1.0, E ** 0.5 / 30)
        if with_b:
            assert float((db.double().cpu() - ref_b).abs().max()) <= 2e-6 * float(ref_b.abs().max() + E ** 0.5)
        else:
            assert torch.isnan(db).all()
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])


@pytest.mark.parametrize("N,E,half,graph", [
    pytest.param(1, 1, False, None, id="1-1-False"), pytest.param(40, 300, False, None, id="40-300-False"),
    pytest.param(5000, 42001, True, None, id="5000-42001-True"), pytest.param(50000, 300001, False, None, id="50000-300001-False"),
    pytest.param(50000, 300001, True, None, id="50000-300001-True"), pytest.param(3000, 2500, False, None, id="3000-2500-False"),
    pytest.param(45, 820, False, "ladder", id="ladder"), pytest.param(300, 2000, False, "hub1000", id="hub1000")])
def test_bn_apply_edge_sums_equals_apply_then_sums(N, E, half, graph):
    """yolat_bn_apply_edge_sums + yolat_edge_uv_sums_v (edge_ops.hip, round 4) against the three launches they replace —
    yolat_bn_relu_bwd_apply, yolat_edge_uv_sums, yolat_edge_attr_dw (torch_vertex.py:331-332 backward): dH1 and dUV
    BIT-identical (same arithmetic, same ascending row order per node; bf16 storage: sums of the stored values), dWc4 /
    db1 against fp64 of the stored dH1 (their summation order differs from k_attr_dw's).  Skewed in-degrees incl. empty
    rows ((3000, 2500): most nodes have no edge); run-to-run bit identity.  `graph` names a graph of graph_ref.GRAPHS in
    place of the squared-uniform draw: the ladder (in-degree n at node n = 0..40: a wave's eight-row trips end inside a
    node at every offset) and hub1000 (a workgroup owns 16 nodes, one of them with 1000 of its ~1090 rows: all four
    quarter boundaries of the workgroup's row range fall inside that node, so two of its waves own no node)."""
    yv = _yv()
    ops = yv.ops
    if graph is None:
        rng = np.random.default_rng(N + E)
        src = rng.integers(0, N, size=E).astype(np.int64)
        dst = (rng.integers(0, N, size=E) ** 2 // max(N, 1)).astype(np.int64)
    else:
        n, src, dst = gr.GRAPHS[graph]()
        assert (n, len(src)) == (N, E)
    gen = torch.Generator().manual_seed(E)
    attr = (torch.randn(E, 4, generator=gen) * (torch.rand(E, 1, generator=gen) > 0.85)).contiguous().cuda()
    g = ops.build_graph(dev(np.stack([src, dst], 1)), attr, None, N, 1)
    g.ensure_csc()
    dt = torch.bfloat16 if half else torch.float32
    H1 = (torch.randn(E, 64, generator=gen) * 1.5 + 0.3).to(dt).cuda()
    dA = torch.randn(E, 64, generator=gen).to(dt).cuda()
    mean = torch.randn(64, generator=gen).cuda() * 0.2
    invstd = (torch.rand(64, generator=gen) + 0.5).cuda()
    gamma = (torch.rand(64, generator=gen) + 0.5).cuda()
    scale = gamma * invstd
    shift = torch.randn(64, generator=gen).cuda() * 0.1 - mean * scale
    coef = (torch.randn(128, generator=gen) * 0.01).cuda()
    # ---- the three launches
    dH_ref = dA.clone()
    ops.bn_relu_bwd_apply(dH_ref, H1, mean, invstd, scale, shift, True, coef, dH_ref)
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    st = torch.cuda.current_stream().cuda_stream
    dUV_ref = torch.empty(N, 128, device="cuda")
    if half:
        check(lib.yolat_edge_uv_sums_h(dH_ref.data_ptr(), 64, g.row_ptr.data_ptr(), g.col_ptr.data_ptr(), g.slots.data_ptr(),
                                       N, 64, dUV_ref.data_ptr(), 128, st))
    else:
        check(lib.yolat_edge_uv_sums(dH_ref.data_ptr(), 64, g.row_ptr.data_ptr(), g.col_ptr.data_ptr(), g.slots.data_ptr(),
                                     N, 64, dUV_ref.data_ptr(), 128, st))
    ref_w = dH_ref.double().cpu().t() @ g.attr[:E].double().cpu()
    ref_b = dH_ref.double().cpu().sum(0)
    # ---- fused
    outs = []
    for _ in range(2):
        dH = dA.clone()
        db = torch.full((64,), float("nan"), device="cuda")
        dUV, dwc4 = ops.bn_apply_edge_sums(dH, H1, mean, invstd, scale, shift, True, coef, g, db)
        dUV[:, 64:] = float("nan")
        check(lib.yolat_edge_uv_sums_v(dH.data_ptr(), 64, int(half), g.col_ptr.data_ptr(), g.slots.data_ptr(), N, 64,
                                       dUV.data_ptr(), 128, st))
        outs.append((dH, dUV, dwc4, db))
    dH, dUV, dwc4, db = outs[0]
    assert torch.equal(dH, dH_ref)
    assert torch.equal(dUV, dUV_ref)
    # ---- and against an fp64 restatement of the op itself (autograd of torch_nn.py:58-66 on the rows, then the two
    # per-node sums of torch_vertex.py:331's factorised backward), not only against the kernels it replaced:
    #   dH = scale (dA [z > 0] - c1 - xhat c2),  z = H1 scale + shift,  xhat = (H1 - mean) invstd
    Yd, dZd = H1.double(), dA.double()
    z = Yd * scale.double() + shift.double()
    xhat = (Yd - mean.double()) * invstd.double()
    want_dH = scale.double() * (dZd * (z > 0) - coef[:64].double() - xhat * coef[64:].double())
    sure = z.abs() > 1e-4                                   # (an activation on the ReLU kink may mask either way in fp32)
    tol = (2.0 ** -7 if half else 2e-6) * want_dH.abs() + (2e-2 if half else 2e-5)
    assert bool((((dH.double() - want_dH).abs() <= tol) | ~sure).all())
    stored = dH.double()
    want_dU = torch.zeros(N, 64, dtype=torch.float64, device="cuda").index_add_(0, g.dst[:E].long(), stored)
    want_dV = torch.zeros(N, 64, dtype=torch.float64, device="cuda").index_add_(0, g.src[:E].long(), stored)
    mag = torch.zeros(N, 64, dtype=torch.float64, device="cuda").index_add_(0, g.dst[:E].long(), stored.abs()) + \
        torch.zeros(N, 64, dtype=torch.float64, device="cuda").index_add_(0, g.src[:E].long(), stored.abs())
    assert bool(((dUV[:, :64].double() - want_dU).abs() <= 4e-6 * mag + 1e-6).all())
    assert bool(((dUV[:, 64:].double() - want_dV).abs() <= 4e-6 * mag + 1e-6).all())
    assert float((dwc4.double().cpu() - ref_w).abs().max()) <= 2e-6 * max(float(ref_w.abs().max()), 1e-3) * max(1.0, E ** 0.5 / 30)
    assert float((db.double().cpu() - ref_b).abs().max()) <= 2e-6 * float(ref_b.abs().max() + E ** 0.5)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,pro", [(65536, True), (70001, True), (70001, False), (131072 + 33, True)])
def test_linear64_row_stream_is_bit_identical_to_the_tile_kernel(M, pro):
    """k_lin64_stream (dense.hip, round 4; taken by yolat_linear_fwd for K = Nout = 64, M >= 65536 with statistics: the
    second edge Linear of a training conv layer, torch_vertex.py:331 nn.3) against the generic 64 x 64 tile kernel run on
    row ranges below the threshold (48 000 rows: a multiple of 32, the statistics' group size): outputs and (sum, M2)
    statistics BIT-identical, ragged last tile included; fp64 check of the product."""
    yv = _yv()
    ops = yv.ops
    gen = torch.Generator().manual_seed(M)
    A = torch.randn(M, 64, generator=gen).cuda()
    W = (torch.randn(64, 64, generator=gen) / 8).cuda()
    b = torch.randn(64, generator=gen).cuda()
    sc = (torch.rand(64, generator=gen) + 0.5).cuda() if pro else None
    sh = torch.randn(64, generator=gen).cuda() * 0.3 if pro else None
    apro = (sc, sh) if pro else None
    Y = torch.full((M, 64), float("nan"), device="cuda")
    st = ops.stats_buffer(M, 64, A.device)
    st.fill_(float("nan"))
    ops.linear_fwd(A, W, b, Y, a_pro=apro, a_relu=pro, stats=st)
    parts_y, parts_s = [], []
    for lo in range(0, M, 48000):
        hi = min(lo + 48000, M)
        Yp = torch.empty(hi - lo, 64, device="cuda")
        sp = ops.stats_buffer(hi - lo, 64, A.device)
        ops.linear_fwd(A[lo:hi], W, b, Yp, a_pro=apro, a_relu=pro, stats=sp)
        parts_y.append(Yp)
        parts_s.append(sp.view(-1)[:2 * 64 * ((hi - lo + 31) // 32)])
    assert torch.equal(Y, torch.cat(parts_y))
    ngrp = (M + 31) // 32
    assert torch.equal(st.view(-1)[:2 * 64 * ngrp], torch.cat(parts_s))
    Ain = torch.relu(A.double() * sc.double() + sh.double()) if pro else A.double()
    ref = Ain @ W.double().t() + b.double()
    assert float((Y.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    # the BatchNorm partial statistics against fp64 too: per 32-row group (sum, M2 about the group's mean) of the
    # pre-epilogue values — what yolat_bn_finalize reduces (include/yolat_hip.h, yolat_linear_fwd)
    pad = ngrp * 32 - M
    refp = torch.cat([ref, torch.zeros(pad, 64, dtype=torch.float64, device="cuda")]) if pad else ref
    valid = torch.cat([torch.ones(M, 1, dtype=torch.float64, device="cuda"),
                       torch.zeros(pad, 1, dtype=torch.float64, device="cuda")]) if pad else torch.ones(M, 1, dtype=torch.float64, device="cuda")
    grp = refp.view(ngrp, 32, 64)
    vg = valid.view(ngrp, 32, 1)
    cnt = vg.sum(1)
    want_sum = (grp * vg).sum(1)
    want_m2 = (((grp - want_sum[:, None, :] / cnt[:, None, :]) ** 2) * vg).sum(1)
    got = st.view(-1)[:2 * 64 * ngrp].view(ngrp, 64, 2).double()
    assert float((got[..., 0] - want_sum).abs().max()) <= 2e-5 * float(want_sum.abs().max())
    assert float((got[..., 1] - want_m2).abs().max()) <= 1e-4 * float(want_m2.abs().max())


@pytest.mark.parametrize("M,K,acc", [(70001, 64, False), (70001, 64, True), (131072 + 33, 128, True), (65536, 128, False)])
def test_linear_fwd_wt_row_stream_is_bit_identical_to_the_tile_kernel(M, K, acc):
    """yolat_linear_fwd_wt for Nout = 64, K in {64, 128}, M >= 65536 on the row-stream kernel (dense.hip k_lin64_stream<KH,
    WT, ACC>: the input-gradient Linears of the training backward over the N nodes — lin_r / mlp_node backward,
    torch_vertex.py:325-327, and dx += dUV . Wuv of the factorised edge Linear) against the generic tile kernel run on row
    ranges below the threshold: BIT-identical with and without accumulation (same products in the same order, the
    epilogue's (acc) + old); fp64 check of the product."""
    yv = _yv()
    ops = yv.ops
    gen = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=gen).cuda()
    Wt = (torch.randn(K, 64, generator=gen) / 8).cuda()
    Y0 = torch.randn(M, 64, generator=gen).cuda()
    Y = Y0.clone()
    ops.linear_fwd_wt(A, Wt, Y, accumulate=acc)
    parts = []
    for lo in range(0, M, 48000):
        hi = min(lo + 48000, M)
        Yp = Y0[lo:hi].clone()
        ops.linear_fwd_wt(A[lo:hi], Wt, Yp, accumulate=acc)
        parts.append(Yp)
    assert torch.equal(Y, torch.cat(parts))
    ref = A.double() @ Wt.double() + (Y0.double() if acc else 0)
    assert float((Y.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
