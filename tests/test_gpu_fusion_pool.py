"""The per-proposal max of the fusion block (`scatter(max)`, arch:122) against float64 references at the layouts of
tests/segmax_layouts.py, on every path the drivers select.

Training (ops.fusion_pool_train_fwd / _bwd, csrc/fusion_train.hip), one parametrised case per mode x layout:
  fp32       F = 1024: x6 rows kernel with the key64 epilogue (fusion_x6.hip), k_gram128, two-term k_fus_da_mfma<32>
  fp32_f160  F = 160 (F % 64 == 32): generic k_gemm_nt with the key64 epilogue (gemm_nt.hpp; a half-masked column tile)
             and the fp32 dA scatter k_fus_da_sparse<8, 256>
  strict     F = 1024 under YOLAT_STRICT_FP32=1, read once per process: ONE child process runs every layout (k_gemm_nt
             key64 epilogue, k_fus_da_sparse) and each case reads its layout's result
  bf16       F = 1024 and bf16_f192 (F = 192): "bf16_dense", k_bt_fusion_rows (bf16_train.hip) + k_fus_da_mfma<32, true>
The reference is float64 autograd on the CPU of Linear -> BatchNorm1d(train) -> ReLU -> oracle scatter(max), whose
_ScatterMax routes a proposal's gradient to the FIRST row among equal maxima (torch_scatter).  The inputs carry
  * exact ties: the proposals of segmax_layouts.tie_proposals (one across a 64-row edge, one across a 256-row edge) hold
    bit-identical copies of one row, so every column ties over the whole proposal; the lowest row must take the gradient,
    checked in dA directly: the first copy carries the scatter term, the other copies only the dense part;
  * gamma == +0 and gamma == -0.0 columns with beta > 0: every row has the activation beta, the first row is the arg and
    dgamma = sum_p g * xhat[first row];
  * negative gammas, and columns closed everywhere (beta = -50: pooled 0, no gradient);
  * near-ties that were not designed (top two activations within 1e-5 relative, not equal, or the largest
    pre-activation within 1e-5 relative of the ReLU's 0: at P x F = 67 M maxima a few sit there) taken out of gZ as in
    test_gpu_ops.py's fusion test; designed ties (exactly equal) are never taken out.
Every mode checks pooled values, running mean / var, dW, dgamma, dbeta, db == 0 and dA accumulated into a non-zero dA; the
Z columns past F stay NaN; backward parts 1, 2 (second stream, ordered by an event), 4 equal parts 7 bit for bit, and
two runs of forward + backward are bit-identical.

bf16 contract (fus_train_fwd / fus_train_bwd_parts with bf16 != 0), restated by _reference(bf16=True):
  * z for routing and for the pooled values comes from the bf16 round-to-nearest-even images of A and W (the products
    exact; summed in float64 here, fp32 in the kernel) plus the fp32 bias;
  * the BatchNorm statistics and running buffers come from the unrounded A and W;
  * the backward evaluates the fp32 formulas of fus_train_bwd_parts at the routed rows: dgamma with xhat from the rounded
    z, dW's gather term and the dense terms of dW and dA from the unrounded A and W — the autograd of
    z_used = z + (z_bf16 - z).detach() — except dA's scatter term, formed from bf16(GM) x bf16(W^T), GM = scale * g in
    fp32 rounded to nearest even.  The reference forms that GM with the kernel's fp32 scale (coef[0]) and the same IEEE
    product, so both sides round the same fp32 values: a GM within fp32 noise of a bf16 rounding midpoint (about 1 in 70
    entries at 3e-5) would otherwise round the other way and move its row by 2^-8 of the product.
With the rounding modelled, what remains is fp32 accumulation, so the bf16 modes are held to the fp32 bound.
Bounds: 2e-4 of each tensor's maximum (pooled, dW, dgamma, dbeta, dA) and 1e-4 (running buffers), those of
test_gpu_ops.py's fusion test.  One exception, at N = 2 only: BatchNorm then leaves dW and dA of O(eps), the difference
of O(1) terms, so there their scale is the largest of the three terms the kernel sums into them (sparse, q1, nq2), 110 x
(bf16, where the rounded xhat is not +-1) to 2000 x (fp32) their own maximum.  Every other layout is held to 2e-4 of the
tensor's maximum.  At N = 2 the columns whose variance the Gram-matrix statistics cannot resolve to fp32
(_resolved_columns) get no upstream gradient; no other layout has one.  Checked by hand with the float64 reference while
writing this file: routing ONE (proposal, column) to another row of its proposal moves, on the `random` layout
(F = 1024), dW by 4.3e-3, dA by 7.3e-3 and dgamma by 3.6e-2 of their maxima, and dgamma by 3.0e-2 for a gamma == 0
column (dW and dA do not move there); on `straddle` (F = 160), dW by 1.7e-2, dA by 3.2e-2 and dgamma by 6.0e-3: at
least 21 x the bound (dW on `random`).

Eval (test_fusion_pair_eval_vs_fp64): yolat_fusion_pair_eval (fp32 MFMA) and yolat_fusion_pair_eval_x6 (bf16x6 rows
kernel with the FX_NP LDS table) at the same layouts, D = 64 and D = 128 (different row tiles, FxShape), against float64
index_reduce_(amax) with empty proposals at 0: values only (the eval kernels return no arg).  The bf16 eval rows kernel
(fusion_h8.hip) and the other routes of the bf16 fusion pair: tests/test_gpu_bf16_eval_stages.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segmax_layouts as sl
from oracle import oracle_torch as orc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 128
EPS, MOM = 1e-5, 0.1
TOL = 2e-4                    # fp32 paths, relative to each tensor's maximum
TOL_RUNNING = 1e-4
MODES = {"fp32": (1024, False), "fp32_f160": (160, False), "bf16": (1024, True), "bf16_f192": (192, True)}


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _bf16(t):
    """float64 image of the bf16 round-to-nearest-even of fp32(t)"""
    return t.float().bfloat16().double()


def _inputs(lay, F):
    tg = torch.Generator().manual_seed(1009 * sl.NAMES.index(lay.name) + F)
    N, P = lay.N, lay.P
    A = torch.relu(torch.randn(N, K, generator=tg)) + 0.3 * torch.rand(1, K, generator=tg)
    st = sl.starts(lay)
    for p in sl.tie_proposals(lay):
        A[st[p]:st[p] + lay.sizes[p]] = A[st[p]].clone()
    W = torch.randn(F, K, generator=tg) / K ** 0.5
    b = torch.randn(F, generator=tg) * 0.1
    gamma = torch.rand(F, generator=tg) * 1.5 - 0.4                  # about a quarter negative
    beta = torch.randn(F, generator=tg) * 0.2
    gamma[0::16] = 0.0
    gamma[1::16] = -0.0
    beta[0::16] = 0.2 + torch.rand(len(range(0, F, 16)), generator=tg)
    beta[1::16] = 0.2 + torch.rand(len(range(1, F, 16)), generator=tg)
    beta[2::16] = -50.0                                                # closed for every row
    assert bool(torch.signbit(gamma[1])) and not bool(torch.signbit(gamma[0]))
    return dict(A=A, W=W, b=b, gamma=gamma, beta=beta,
                rm=torch.randn(F, generator=tg) * 0.1, rv=1.0 + torch.rand(F, generator=tg),
                gZ=torch.randn(P, F, generator=tg) / P ** 0.5, d_in=torch.randn(N, K, generator=tg) * 0.01)


def _scatter_rows(M, arg, N):
    """[P, F] entries to their arg rows -> [N, F] (arg == N: empty proposal, dropped)"""
    out = torch.zeros(N + 1, M.shape[1], dtype=M.dtype)
    out.scatter_(0, arg, M)
    return out[:N]


def _resolved_columns(inp):
    """Columns whose batch variance the Gram-matrix statistics resolve to fp32 accuracy.  var_c = w_c G w_c^T / N carries
    fp32 error ~ kappa_c 2^-24 K, kappa_c = sum_r (|A_r - mean| . |w_c|)^2 / sum_r ((A_r - mean) . w_c)^2: at N = 2 a
    column whose two z nearly coincide has kappa up to 1e8 (by design of the statistics, not a routing question).  Such a
    column gets no upstream gradient, like a near-tie; no layout but N = 2 has one (check_training asserts it)."""
    Ac = inp["A"].double() - inp["A"].double().mean(0)
    W = inp["W"].double()
    return (Ac.abs() @ W.abs().t()).pow(2).sum(0) < 1e3 * (Ac @ W.t()).pow(2).sum(0)


def _reference(lay, inp, bf16):
    N, P = lay.N, lay.P
    idx = torch.from_numpy(lay.bbox_idx)
    A, W = inp["A"].double(), inp["W"].double()
    A64, W64 = A.clone().requires_grad_(True), W.clone().requires_grad_(True)
    b64 = inp["b"].double().requires_grad_(True)
    g64 = inp["gamma"].double().requires_grad_(True)
    be64 = inp["beta"].double().requires_grad_(True)
    z = A64 @ W64.t() + b64
    # a BLAS may sum the rows of one product in different orders (edge micro-tiles): give the copies of a tie proposal
    # exactly their first row's z (a change within an ulp; the gradient still flows to each copy's own row)
    st = sl.starts(lay)
    with torch.no_grad():
        zc = z.detach().clone()
        for p in sl.tie_proposals(lay):
            zc[st[p] + 1:st[p] + lay.sizes[p]] = zc[st[p]]
    z = z + (zc - z).detach()
    mean, var = z.mean(0), z.var(0, unbiased=False)
    if bf16:
        with torch.no_grad():
            zr = _bf16(A) @ _bf16(W).t() + inp["b"].double()
            for p in sl.tie_proposals(lay):
                zr[st[p] + 1:st[p] + lay.sizes[p]] = zr[st[p]]
        z = z + (zr - z).detach()
    rstd = 1.0 / torch.sqrt(var + EPS)
    pre = (z - mean) * rstd * g64 + be64
    y = torch.relu(pre)
    pooled, arg = orc._ScatterMax.apply(y, idx, P)
    with torch.no_grad():
        top0 = pooled.detach()
        rows = torch.arange(N).view(-1, 1)
        others = y.detach().masked_fill(arg.index_select(0, idx) == rows, float("-inf"))
        top1 = torch.full((P, y.shape[1]), float("-inf"), dtype=torch.float64).scatter_reduce(
            0, idx.view(-1, 1).expand_as(others), others, "amax", include_self=True)
        near = (top0 > 0) & (top1 < top0) & ((top0 - top1) < 1e-5 * (top0.abs() + 1e-3))
        # the same at the ReLU gate: a proposal's largest pre-activation within fp32 rounding of 0 (tie with the floor)
        pmax = torch.full_like(top0, float("-inf")).scatter_reduce(0, idx.view(-1, 1).expand_as(pre), pre.detach(),
                                                                   "amax", include_self=True)
        beta = be64.detach()
        near |= pmax.abs() < 1e-5 * ((pmax - beta).abs() + beta.abs() + 1e-3)
        near |= ~_resolved_columns(inp)[None, :]
        gZ = inp["gZ"].double().masked_fill(near, 0.0)
    pooled.backward(gZ)
    with torch.no_grad():
        gm = gZ * (top0 > 0)                                  # g masked by the ReLU at the arg row
        ref = dict(pooled=top0, arg=arg, gm=gm, dW=W64.grad, db=b64.grad, dgamma=g64.grad, dbeta=be64.grad,
                   dA=A64.grad, rm=(1 - MOM) * inp["rm"].double() + MOM * mean,
                   rv=(1 - MOM) * inp["rv"].double() + MOM * var * N / (N - 1))
        GM = _scatter_rows(gm * (g64 * rstd), arg, N)          # dL/dz at the arg rows, GM = scale * g
        ref["scatter"] = GM @ W                                   # dA's scatter term
        # the terms fus_train_bwd_parts sums into dW and dA (fusion_train.hip's header): the sparse ones, q1 = s dbeta / N
        # times sum_r A_r (dW) or W (dA), nq2 = -s rstd dgamma / N times W G (dW) or (A - mean_A) W^T diag(nq2) W (dA)
        sc = (g64 * rstd).detach()
        q1, nq2 = sc * be64.grad / N, -sc * rstd.detach() * g64.grad / N
        Ac = A - A.mean(0)
        ref["dW_terms"] = torch.stack([(GM.t() @ A).abs().max(), (q1[:, None] * A.sum(0)).abs().max(),
                                       (nq2[:, None] * (W @ (Ac.t() @ Ac))).abs().max()])
        ref["dA_terms"] = torch.stack([ref["scatter"].abs().max(), (q1 @ W).abs().max(),
                                       (Ac @ (W.t() @ (nq2[:, None] * W))).abs().max()])
    return ref, gZ.float()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_gpu(lay, inp, gZ, F, bf16):
    yv = _yv()
    N, P = lay.N, lay.P
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(),
                           torch.from_numpy(lay.bbox_idx).cuda(), N, P)
    A, gZd = inp["A"].cuda(), gZ.cuda()

    def fwd():
        lin, bn = torch.nn.Linear(K, F).cuda(), torch.nn.BatchNorm1d(F, eps=EPS, momentum=MOM).cuda()
        with torch.no_grad():
            for dst, key in ((lin.weight, "W"), (lin.bias, "b"), (bn.weight, "gamma"), (bn.bias, "beta"),
                             (bn.running_mean, "rm"), (bn.running_var, "rv")):
                dst.copy_(inp[key])
        Zbuf = torch.full((P, F + 64), float("nan")).cuda()
        sv = yv.ops.fusion_pool_train_fwd(A, lin, bn, g, Zbuf[:, :F], bf16=bf16)
        return sv, Zbuf, bn

    side_stream = torch.cuda.Stream()

    def side(fn, keep):
        side_stream.wait_stream(torch.cuda.current_stream())          # an event recorded behind part 1
        with torch.cuda.stream(side_stream):
            fn()

    def bwd(sv, split):
        dW, db = torch.full((F, K), float("nan")).cuda(), torch.full((F,), float("nan")).cuda()
        dg, dbt = torch.full((F,), float("nan")).cuda(), torch.full((F,), float("nan")).cuda()
        dA = inp["d_in"].cuda()
        yv.ops.fusion_pool_train_bwd(sv, g, gZd, dW, db, dg, dbt, dA, side=side if split else None)
        if split:
            torch.cuda.current_stream().wait_stream(side_stream)
        return dict(dW=dW.cpu(), db=db.cpu(), dgamma=dg.cpu(), dbeta=dbt.cpu(), dA=dA.cpu())

    sv1, Z1, bn1 = fwd()
    sv2, Z2, bn2 = fwd()
    out = dict(Z=Z1.cpu(), scale=sv1["coef"][0].cpu(), rm=bn1.running_mean.cpu(), rv=bn1.running_var.cpu(), grads=bwd(sv1, False),
               split=bwd(sv1, True), rerun=bwd(sv2, False))
    torch.cuda.synchronize()
    assert torch.equal(_bits(Z1[:, :F]), _bits(Z2[:, :F])), "forward not deterministic"
    assert torch.equal(_bits(bn1.running_mean), _bits(bn2.running_mean))
    assert torch.equal(_bits(bn1.running_var), _bits(bn2.running_var))
    for k, v in out["grads"].items():
        assert torch.equal(_bits(v), _bits(out["split"][k])), ("parts 1, 2 (side stream), 4 != parts 7", k)
        assert torch.equal(_bits(v), _bits(out["rerun"][k])), ("backward not deterministic", k)
    return out


def _rel(got, want, name, errs, tol=TOL, term=None):
    """worst |got - want| relative to max |want|, or to the largest term the kernel sums into it when `term` is given
    (dW and dA at N = 2 only: BatchNorm leaves a gradient of O(eps), the difference of O(1) terms)"""
    got, want = got.double(), want.double()
    scale = max(float(want.abs().max()), float(term.abs().max()) if term is not None else 0.0, 1e-30)
    worst = float((got - want).abs().max()) / scale
    errs[name] = worst
    assert bool(torch.isfinite(got).all()) and worst < tol, (name, worst, tol)


def check_training(name, F, bf16):
    """one layout in one mode; returns the worst relative errors"""
    lay = sl.layout(name)
    inp = _inputs(lay, F)
    ref, gZ = _reference(lay, inp, bf16)
    got = _run_gpu(lay, inp, gZ, F, bf16)
    if bf16:
        # dA's scatter term on bf16(GM) x bf16(W^T): GM = fp32(scale * g) with the kernel's fp32 scale (coef[0], the
        # same IEEE product as k_fus_cols_partial's), so that both sides round the same fp32 values
        W = inp["W"].double()
        GM = (ref["gm"].float() * got["scale"]).double()
        sb = _scatter_rows(_bf16(GM), ref["arg"], lay.N) @ _bf16(W)
        ref["dA"], ref["scatter"] = ref["dA"] - ref["scatter"] + sb, sb
    errs = {}
    Z = got["Z"]
    assert bool(torch.isnan(Z[:, F:]).all()), "Z columns past F were written"
    _rel(Z[:, :F], ref["pooled"], "pooled", errs)
    empty = torch.from_numpy(lay.sizes == 0)
    assert float(Z[empty, :F].abs().max()) == 0.0 if bool(empty.any()) else True
    assert float(Z[:, 2:F:16].abs().max()) == 0.0                        # closed columns
    _rel(got["rm"], ref["rm"], "running_mean", errs, TOL_RUNNING)
    _rel(got["rv"], ref["rv"], "running_var", errs, TOL_RUNNING)
    gr = got["grads"]
    assert float(gr["db"].abs().max()) == 0.0 and float(ref["db"].abs().max()) < 1e-9
    assert bool(_resolved_columns(inp).all()) or lay.N == 2
    n2 = lay.N == 2
    _rel(gr["dW"], ref["dW"], "dW", errs, term=ref["dW_terms"] if n2 else None)
    _rel(gr["dgamma"], ref["dgamma"], "dgamma", errs)
    _rel(gr["dbeta"], ref["dbeta"], "dbeta", errs)
    d_in = inp["d_in"].double()
    dA = gr["dA"].double() - d_in
    _rel(dA, ref["dA"], "dA", errs, term=ref["dA_terms"] if n2 else None)
    # gamma == +-0 columns: routed to the first row, so dgamma follows xhat there; they carry no dz
    zc = torch.cat([torch.arange(0, F, 16), torch.arange(1, F, 16)])
    assert float(ref["dgamma"][zc].abs().max()) > 0.0 and float(ref["dW"][zc].abs().max()) == 0.0
    # exact ties: the first copy carries the scatter term, every other copy only the dense part
    st = sl.starts(lay)
    scale = float(ref["dA"].abs().max())
    for p in sl.tie_proposals(lay):
        lo, hi = int(st[p]), int(st[p] + lay.sizes[p])
        assert int(ref["arg"][p].min()) == lo and int(ref["arg"][p].max()) == lo
        assert float(ref["scatter"][lo + 1:hi].abs().max()) == 0.0
        want = ref["scatter"][lo]
        assert float(want.abs().max()) > 100 * TOL * scale
        dense = dA[lo + 1]
        assert float((dA[lo + 1:hi] - dense).abs().max()) <= 1e-5 * scale, ("tie copies differ", p)
        assert float(((dA[lo] - dense) - want).abs().max()) <= TOL * scale, ("tie row", p)
    return errs


CASES = [(name, mode) for name in sl.NAMES for mode in MODES]


@pytest.mark.parametrize("name,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_fusion_pool_train_vs_fp64(name, mode):
    F, bf16 = MODES[mode]
    errs = check_training(name, F, bf16)
    print("%s %s: %s" % (mode, name, " ".join("%s %.2e" % kv for kv in errs.items())))


def _strict_child(out_path):
    """every layout under YOLAT_STRICT_FP32=1 (set by the parent before this process started)"""
    assert os.environ.get("YOLAT_STRICT_FP32") == "1"
    res = {}
    for name in sl.NAMES:
        try:
            res[name] = {"errs": check_training(name, 1024, False)}
        except AssertionError as e:
            res[name] = {"error": repr(e)}
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def strict_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("strict") / "strict.json")
    script = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_fusion_pool as t\nt._strict_child(sys.argv[1])\n"
              % (REPO, os.path.join(REPO, "tests")))
    subprocess.run([sys.executable, "-c", script, out], check=True, timeout=480,
                   env=dict(os.environ, YOLAT_STRICT_FP32="1"))
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sl.NAMES)
def test_fusion_pool_train_strict_fp32_vs_fp64(name, strict_results):
    r = strict_results[name]
    assert "error" not in r, r.get("error")
    print("strict %s: %s" % (name, " ".join("%s %.2e" % kv for kv in r["errs"].items())))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", sl.NAMES)
def test_fusion_pair_eval_vs_fp64(name, D):
    """yolat_fusion_pair_eval and yolat_fusion_pair_eval_x6: pooled = max over a proposal's rows of
    relu((A W^T + b) * s + t), 0 for an empty proposal; tie proposals, s == +-0 columns (t > 0), negative s and closed
    columns as in the training cases.  Bound: 4e-6 of the largest pooled value (fp32-class GEMMs; the x6 test of
    test_gpu_ops.py holds 2e-6 / 3e-6 on random data)."""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    lay = sl.layout(name)
    N, P, F = lay.N, lay.P, 512
    tg = torch.Generator().manual_seed(7 * sl.NAMES.index(name) + D)
    A = torch.relu(torch.randn(N, D, generator=tg)) + 0.3 * torch.rand(1, D, generator=tg)
    st = sl.starts(lay)
    for p in sl.tie_proposals(lay):
        A[st[p]:st[p] + lay.sizes[p]] = A[st[p]].clone()
    Wf, Wfs = torch.randn(F, D, generator=tg) / D ** 0.5, torch.randn(F, D, generator=tg) / D ** 0.5
    bf, bfs = torch.randn(F, generator=tg) * 0.1, torch.randn(F, generator=tg) * 0.1
    sf, sfs = torch.rand(F, generator=tg) - 0.3, torch.rand(F, generator=tg) + 0.5
    tf, tfs = torch.randn(F, generator=tg) * 0.2, torch.randn(F, generator=tg) * 0.2
    sf[0::16], sf[1::16] = 0.0, -0.0
    tf[0::16], tf[1::16] = 0.4, 0.7
    tf[2::16] = -50.0
    S = torch.randn(P, D, generator=tg)
    want = torch.zeros(P, F, dtype=torch.float64)
    act = torch.relu((A.double() @ Wf.double().t() + bf.double()) * sf.double() + tf.double())
    want.index_reduce_(0, torch.from_numpy(lay.bbox_idx), act, "amax", include_self=True)
    Ad, Sd, Wfd, Wfsd = A.cuda(), S.cuda(), Wf.cuda(), Wfs.cuda()
    bfd, sfd, tfd, bfsd, sfsd, tfsd = (t.cuda() for t in (bf, sf, tf, bfs, sfs, tfs))
    seg = torch.from_numpy(lay.bbox_idx).int().cuda()
    st_ = torch.cuda.current_stream().cuda_stream
    ZW = 2 * (F + D)

    def fresh():
        Z = torch.zeros(P, ZW).cuda()
        Z[:, F:F + D] = float("nan")                                   # not written by either kernel
        return Z

    Za = fresh()
    check(lib.yolat_fusion_pair_eval(Ad.data_ptr(), D, N, D, Wfd.data_ptr(), bfd.data_ptr(), sfd.data_ptr(),
                                     tfd.data_ptr(), F, seg.data_ptr(), Za.data_ptr(), ZW, Sd.data_ptr(), D, P,
                                     Wfsd.data_ptr(), bfsd.data_ptr(), sfsd.data_ptr(), tfsd.data_ptr(),
                                     Za[:, F + D:].data_ptr(), ZW, st_))
    parts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    sparts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    check(lib.yolat_split_bf16x3(Wfd.data_ptr(), D, F, D, sfd.data_ptr(), *(t.data_ptr() for t in parts), st_))
    check(lib.yolat_split_bf16x3(Wfsd.data_ptr(), D, F, D, sfsd.data_ptr(), *(t.data_ptr() for t in sparts), st_))
    tfold, tsfold = sfd * bfd + tfd, sfsd * bfsd + tfsd
    Zb = fresh()
    check(lib.yolat_fusion_pair_eval_x6(Ad.data_ptr(), D, N, D, *(t.data_ptr() for t in parts), tfold.data_ptr(), F,
                                        seg.data_ptr(), Zb.data_ptr(), ZW, Sd.data_ptr(), D, P,
                                        *(t.data_ptr() for t in sparts), tsfold.data_ptr(), Zb[:, F + D:].data_ptr(), ZW,
                                        st_))
    torch.cuda.synchronize()
    scale = float(want.abs().max())
    empty = torch.from_numpy(lay.sizes == 0)
    for tag, Z in (("fp32", Za), ("x6", Zb)):
        Z = Z.cpu()
        assert bool(torch.isnan(Z[:, F:F + D]).all()), tag
        err = float((Z[:, :F].double() - want).abs().max()) / scale
        print("eval %s D=%d %s: %.2e" % (tag, D, name, err))
        assert err <= 4e-6, (tag, err)
        assert float(Z[:, 2:F:16].abs().max()) == 0.0, tag
        if bool(empty.any()):
            assert float(Z[empty, :F].abs().max()) == 0.0, tag


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_misaligned_A_is_declined_before_anything_is_enqueued(bf16):
    """The backward reads A's rows with 16-byte loads (k_fus_dw_sparse), so the training forward and backward both
    decline an A whose base is not 16-byte aligned (YOLAT_E_UNSUPPORTED -> ValueError) before they enqueue anything:
    Z, the running buffers, dW and dA stay as they were."""
    yv = _yv()
    lay = sl.layout("small_n33")
    N, P, F = lay.N, lay.P, 192
    inp = _inputs(lay, F)
    g = yv.ops.build_graph(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.zeros(0, 4).cuda(),
                           torch.from_numpy(lay.bbox_idx).cuda(), N, P)
    buf = torch.zeros(N * K + 4).cuda()
    A_mis = buf[1:1 + N * K].view(N, K)
    A_mis.copy_(inp["A"])
    assert A_mis.data_ptr() % 16 == 4 and A_mis.stride(0) == K
    lin, bn = torch.nn.Linear(K, F).cuda(), torch.nn.BatchNorm1d(F).cuda()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    Zbuf = torch.full((P, F), float("nan")).cuda()
    with pytest.raises(ValueError, match="base address % 16 = 4"):
        yv.ops.fusion_pool_train_fwd(A_mis, lin, bn, g, Zbuf, bf16=bf16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Zbuf).all())
    assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
    # a backward handed the misaligned A (its forward ran on an aligned copy)
    sv = yv.ops.fusion_pool_train_fwd(inp["A"].cuda(), lin, bn, g, Zbuf, bf16=bf16)
    sv["A"] = A_mis
    dW, db = torch.full((F, K), float("nan")).cuda(), torch.full((F,), float("nan")).cuda()
    dg, dbt = torch.full((F,), float("nan")).cuda(), torch.full((F,), float("nan")).cuda()
    dA = inp["d_in"].cuda()
    with pytest.raises(ValueError, match="base address % 16 = 4"):
        yv.ops.fusion_pool_train_bwd(sv, g, inp["gZ"].cuda(), dW, db, dg, dbt, dA)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(dg).all()) and bool(torch.isnan(dbt).all())
    assert torch.equal(dA.cpu(), inp["d_in"])
