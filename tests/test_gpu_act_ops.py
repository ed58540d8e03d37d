"""GPU tests, op level: the kernels of csrc/act.hip per element against float64.

  yolat_fusion_pair_eval_act   pooled[p] = max over the rows of proposal p of act(s * (A W^T + b) + t), 0 for an empty
                               proposal; the super half act(ss * (S Ws^T + bs) + ts)  — every layout of segmax_layouts.py
  yolat_scale_shift_act / yolat_bn_act_bwd    forward and backward of act(BN_train(y)), the slope gradient included

Bound of the pooled values: 2e-4 of the tensor maximum, the bar of tests/test_gpu_fusion_pool.py.  The activation is applied
BEFORE the maximum: with slope -0.3 it is not monotone, with 0.2 a column that is negative in every row pools to a negative
value (not to the 0 a ReLU-minded pooling starts from).
"""
import numpy as np
import pytest
import torch

import segmax_layouts as sl

pytestmark = pytest.mark.gpu

TOL = 2e-4


def _act(y, a):
    return torch.where(y > 0, y, a * y)


@pytest.mark.parametrize("slope", [0.2, -0.3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", sl.NAMES)
def test_fusion_pair_eval_act_vs_fp64(name, D, slope):
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    lay = sl.layout(name)
    N, P, F = lay.N, lay.P, 512
    tg = torch.Generator().manual_seed(11 * sl.NAMES.index(name) + D)
    A = torch.relu(torch.randn(N, D, generator=tg)) + 0.3 * torch.rand(1, D, generator=tg)
    st = sl.starts(lay)
    for p in sl.tie_proposals(lay):
        A[st[p]:st[p] + lay.sizes[p]] = A[st[p]].clone()
    Wf, Wfs = torch.randn(F, D, generator=tg) / D ** 0.5, torch.randn(F, D, generator=tg) / D ** 0.5
    bf, bfs = torch.randn(F, generator=tg) * 0.1, torch.randn(F, generator=tg) * 0.1
    sf, sfs = torch.rand(F, generator=tg) - 0.25, torch.rand(F, generator=tg) - 0.25      # about a quarter negative
    tf, tfs = torch.randn(F, generator=tg) * 0.2, torch.randn(F, generator=tg) * 0.2
    sf[0::16], sf[1::16] = 0.0, -0.0
    tf[0::16], tf[1::16] = 0.4, -0.7
    tf[2::16] = -50.0                                      # negative in every row
    S = torch.randn(P, D, generator=tg)
    a_f, a_s = torch.tensor([slope]), torch.tensor([-slope])
    y = (A.double() @ Wf.double().t() + bf.double()) * sf.double() + tf.double()
    idx = torch.from_numpy(lay.bbox_idx)
    want = torch.zeros(P, F, dtype=torch.float64)
    want.index_reduce_(0, idx, _act(y, slope), "amax", include_self=False)
    empty = torch.from_numpy(lay.sizes == 0)
    want[empty] = 0.0
    want_s = _act((S.double() @ Wfs.double().t() + bfs.double()) * sfs.double() + tfs.double(), -slope)
    # the inputs do what the case is about
    filled = want[~empty]
    if slope > 0:
        assert float((filled < 0).double().mean()) >= 0.02 and bool((filled[:, 2::16] < 0).all())
    else:
        naive = torch.zeros(P, F, dtype=torch.float64)
        naive.index_reduce_(0, idx, y, "amax", include_self=False)
        big = torch.from_numpy(lay.sizes >= 3)             # (a one-row proposal cannot tell the two orders apart)
        if bool(big.any()):
            assert float((_act(naive, slope)[big] != want[big]).double().mean()) >= 0.05

    seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lay.sizes)]).astype(np.int32)).cuda()
    dev = [t.cuda() for t in (A, S, Wf, Wfs, bf, sf, tf, bfs, sfs, tfs, a_f, a_s)]
    Ad, Sd, Wfd, Wfsd, bfd, sfd, tfd, bfsd, sfsd, tfsd, afd, asd = dev
    ZW = 2 * (F + D)
    Z = torch.full((P, ZW), float("nan"), device="cuda")   # the pooled block is WRITTEN: no zeroed pool needed
    work = torch.empty(int(lib.yolat_fusion_pair_eval_act_work_elems(N, F)), device="cuda")
    assert work.numel() * 4 <= 64 << 20 or work.numel() == N * 64
    check(lib.yolat_fusion_pair_eval_act(Ad.data_ptr(), D, N, D, Wfd.data_ptr(), bfd.data_ptr(), sfd.data_ptr(), tfd.data_ptr(),
                                         F, afd.data_ptr(), seg_ptr.data_ptr(), Z.data_ptr(), ZW, Sd.data_ptr(), D, P,
                                         Wfsd.data_ptr(), bfsd.data_ptr(), sfsd.data_ptr(), tfsd.data_ptr(), asd.data_ptr(),
                                         Z[:, F + D:].data_ptr(), ZW, work.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "yolat_fusion_pair_eval_act")
    # the activation-aware instantiation of the bf16x6 rows kernel: signed atomics on start values it sets itself
    st_ = torch.cuda.current_stream().cuda_stream
    seg = torch.from_numpy(lay.bbox_idx).int().cuda()
    parts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    sparts = [torch.empty(F * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    check(lib.yolat_split_bf16x3(Wfd.data_ptr(), D, F, D, sfd.data_ptr(), *(t.data_ptr() for t in parts), st_))
    check(lib.yolat_split_bf16x3(Wfsd.data_ptr(), D, F, D, sfsd.data_ptr(), *(t.data_ptr() for t in sparts), st_))
    tfold, tsfold = sfd * bfd + tfd, sfsd * bfsd + tfsd
    Zx = torch.full((P, ZW), float("nan"), device="cuda")
    check(lib.yolat_fusion_pair_eval_x6_act(Ad.data_ptr(), D, N, D, *(t.data_ptr() for t in parts), tfold.data_ptr(), F,
                                            afd.data_ptr(), seg.data_ptr(), seg_ptr.data_ptr(), Zx.data_ptr(), ZW,
                                            Sd.data_ptr(), D, P, *(t.data_ptr() for t in sparts), tsfold.data_ptr(),
                                            asd.data_ptr(), Zx[:, F + D:].data_ptr(), ZW, st_),
          "yolat_fusion_pair_eval_x6_act")
    torch.cuda.synchronize()
    for tag, Zt in (("materialising", Z), ("x6", Zx)):
        Zt = Zt.cpu()
        assert bool(torch.isnan(Zt[:, F:F + D]).all()) and bool(torch.isnan(Zt[:, 2 * F + D:]).all()), tag   # not written
        err = float((Zt[:, :F].double() - want).abs().max()) / float(want.abs().max())
        err_s = float((Zt[:, F + D:2 * F + D].double() - want_s).abs().max()) / float(want_s.abs().max())
        print("act pair %s D=%d %s slope %g: pooled %.2e super %.2e" % (tag, D, name, slope, err, err_s))
        assert err <= TOL and err_s <= TOL, tag
        if bool(empty.any()):
            assert float(Zt[empty, :F].abs().max()) == 0.0, tag
        if tag == "materialising":
            # exact where no arithmetic is involved: s == +-0 columns are act(t) in every row
            assert bool((Zt[~empty][:, 0:F:16] == torch.tensor(0.4)).all())
            assert bool((Zt[~empty][:, 1:F:16] == torch.tensor(-0.7) * torch.tensor(slope)).all())
        else:
            # (the folded shift s*b + t of the x6 form is t where s == +-0)
            assert float((Zt[~empty][:, 0:F:16] - 0.4).abs().max()) <= 1e-6
            assert float((Zt[~empty][:, 1:F:16] + 0.7 * slope).abs().max()) <= 1e-6
        if slope > 0:
            assert bool((Zt[~empty][:, 2:F:16] < 0).all()), tag      # negative in every row: pooled negative, not 0


def test_pooling_propagates_nan():
    from yolat_vectorgraphicsrecognition_amd import ops
    Y = torch.randn(40, 70)
    Y[7, 3] = float("nan")
    g = ops.Graph()
    g.P = 3
    g.seg_ptr = torch.tensor([0, 10, 10, 40], dtype=torch.int32).cuda()
    out = torch.empty(3, 70).cuda()
    a = torch.tensor([0.2]).cuda()
    ops.segment_act_max(Y.cuda(), a, g, out)
    out = out.cpu()
    want = _act(Y, 0.2)
    assert bool(torch.isnan(out[0, 3])) and int(torch.isnan(out).sum()) == 1
    keep = torch.ones(70, dtype=torch.bool)
    keep[3] = False
    assert torch.equal(out[0, keep], want[:10].max(0).values[keep])
    assert float(out[1].abs().max()) == 0.0
    assert torch.equal(out[2], want[10:].max(0).values)


@pytest.mark.parametrize("M,C", [(37, 70), (600, 96), (1, 5)])
@pytest.mark.parametrize("slope", [0.2, -0.3, 0.0, 1.3])
def test_bn_act_forward_and_backward_vs_fp64(M, C, slope):
    """act(BN_train(y)) through ops.scale_shift_act / ops.bn_act_bwd against torch autograd in float64: dy, dgamma, dbeta and
    the slope gradient (sum over y' <= 0 of g * y'); rows that are no multiple of the 256-row block, columns that are no
    multiple of 64; two calls give the same bits.  Bound: 1e-5 of each tensor's maximum (fp32 sums of <= 600 terms per
    column accumulated per block, float64 across blocks)."""
    from yolat_vectorgraphicsrecognition_amd import ops
    tg = torch.Generator().manual_seed(M + C)
    y = torch.randn(M, C, generator=tg) * 1.5 + 0.2
    gz = torch.randn(M, C, generator=tg)
    gamma, beta = torch.rand(C, generator=tg) + 0.5, torch.randn(C, generator=tg) * 0.3
    gamma[::5] *= -1.0
    eps = 1e-5
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a64 = torch.tensor([slope], dtype=torch.float64, requires_grad=True)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    yb = (y64 - mean) / torch.sqrt(var + eps) * g64 + b64
    z64 = torch.nn.functional.prelu(yb, a64)
    (z64 * gz.double()).sum().backward()
    invstd = (1.0 / torch.sqrt(var.detach() + eps)).float()
    scale = (gamma.double() * invstd.double()).float()
    shift = (beta.double() - mean.detach() * scale.double()).float()
    dev = [t.cuda() for t in (y, gz, mean.detach().float(), invstd, scale, shift, torch.tensor([slope]))]
    yd, gzd, md, isd, scd, shd, ad = dev
    z = ops.scale_shift_act(yd, scd, shd, ad, torch.empty_like(yd))
    if M > 1:                        # (one row: var = 0, scale = gamma / sqrt(eps) turns fp32 rounding of y into 1e-5 errors)
        assert float((z.cpu().double() - z64.detach()).abs().max()) <= 1e-5 * max(float(z64.detach().abs().max()), 1e-6)

    def run():
        dg, db, da = torch.empty(C).cuda(), torch.empty(C).cuda(), torch.empty(1).cuda()
        dy = ops.bn_act_bwd(gzd.clone(), yd, md, isd, scd, shd, ad, dg, db, da, torch.empty_like(yd))
        return dy, dg, db, da
    got, again = run(), run()
    for t, u in zip(got, again):
        assert torch.equal(t, u)
    if M == 1:
        assert all(bool(torch.isfinite(t).all()) for t in got)
        return                       # (the bits and the tail handling are the point of the one-row case)
    for name, t, w in zip(("dy", "dgamma", "dbeta", "dslope"), got, (y64.grad, g64.grad, b64.grad, a64.grad)):
        err = float((t.cpu().double() - w).abs().max())
        print("%s: %.2e of %.3g" % (name, err, float(w.abs().max())))
        assert err <= 1e-5 * max(float(w.abs().max()), 1e-6) + 1e-6, name
