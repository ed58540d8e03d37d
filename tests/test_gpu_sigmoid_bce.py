"""GPU tests (-m gpu) of the sigmoid / BCELoss kernels (csrc/loss_optim.hip: yolat_sigmoid, yolat_sigmoid_bwd, yolat_bce,
yolat_sigmoid_bce) — the classifier != 'softmax' branch of architecture3cc_rpn_gp_iter2.py:132-133,362-376.

Reference: torch.sigmoid + nn.BCELoss + autograd on the CPU, from the same fp32 logits — in float64 where the inputs stay
clear of saturation (|z| <= 13.7 for randn * 3 at these seeds), and torch's own fp32 ops for the saturation quirk, which is
a property of fp32 rounding (p == 1.0f exactly -> loss term 100, gradient 0).  Tolerance: the op tolerance of
tests/test_gpu_ops.py (rtol 1e-4 of the tensor's scale + of the element); torch's fp32 CPU result sits within 6e-7 (loss),
2.5e-7 of the largest element (gradient) and 9e-8 (probabilities) of float64 on these inputs."""
import pytest
import torch

from test_gpu_ops import close

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _draw(P, K):
    g = torch.Generator().manual_seed(P)
    z = torch.randn(P, K, generator=g) * 3
    y = torch.randint(0, K, (P,), generator=g)
    return z, y


def _torch_ref(z, y, dtype):
    """(prob, loss, dlogits) of torch.sigmoid -> nn.BCELoss against the one-hot labels, on the CPU in `dtype`"""
    zz = z.detach().clone().to(dtype).requires_grad_(True)
    p = torch.sigmoid(zz)
    tgt = torch.zeros(p.size(), dtype=dtype).scatter_(1, y.unsqueeze(1), 1)
    loss = torch.nn.BCELoss()(p, tgt)
    loss.backward()
    return p.detach(), loss.detach().reshape(1), zz.grad


_REF = {}


def _ref64(P, K):
    if (P, K) not in _REF:
        z, y = _draw(P, K)
        _REF[(P, K)] = (z, y) + _torch_ref(z, y, torch.float64)
    return _REF[(P, K)]


def _fused(yv, z_dev, y_dev, want_grad=True, want_prob=True):
    P, K = z_dev.shape
    loss = torch.empty(1, device="cuda")
    dl = torch.empty(P, K, device="cuda") if want_grad else None
    prob = torch.empty(P, K, device="cuda") if want_prob else None
    yv.ops.sigmoid_bce(z_dev, y_dev, loss, dl, prob)
    return prob, loss, dl


def _composed(yv, z_dev, y_dev):
    P, K = z_dev.shape
    loss = torch.empty(1, device="cuda")
    prob = yv.ops.sigmoid(z_dev)
    dp = torch.empty(P, K, device="cuda")
    yv.ops.bce(prob, y_dev, loss, dp)
    dl = yv.ops.sigmoid_bwd(dp, prob)
    return prob, loss, dl


# one row; one partial workgroup; a row count that crosses the 256-row workgroup with K > 32 (the plain-loop kernel);
# twelve workgroups of partials
SHAPES = [(1, 17), (40, 17), (257, 33), (3000, 22)]


@pytest.mark.parametrize("P,K", SHAPES)
def test_sigmoid_bce_against_torch_float64(P, K):
    yv = _yv()
    z, y, p64, loss64, dz64 = _ref64(P, K)
    assert float(z.abs().max()) <= 13.7
    for name, fn in (("fused", _fused), ("composed", _composed)):
        prob, loss, dl = fn(yv, z.cuda(), y.cuda())
        close(prob, p64, msg="%s prob" % name)
        close(loss, loss64, msg="%s loss" % name)
        close(dl, dz64, msg="%s dlogits" % name)
    # the loss alone (no gradient, no probabilities asked for): the same number
    _, loss_only, _ = _fused(yv, z.cuda(), y.cuda(), want_grad=False, want_prob=False)
    assert torch.equal(loss_only, loss)
    loss_b = torch.empty(1, device="cuda")
    yv.ops.bce(prob, y.cuda(), loss_b)
    assert torch.equal(loss_b, loss)


def test_sigmoid_bce_on_a_column_slice_of_a_wider_buffer():
    """ld > K on every operand: logits, probabilities and both gradients are column slices of wider buffers, whose other
    columns must stay untouched"""
    yv = _yv()
    P, K = 40, 17
    z, y, p64, loss64, dz64 = _ref64(P, K)
    wide = torch.full((P, 40), 1e30, device="cuda")
    wide[:, 5:5 + K] = z.cuda()
    zs = wide[:, 5:5 + K]
    outs = {n: torch.full((P, 29), -7.0, device="cuda") for n in ("prob", "dl", "prob2", "dp", "dl2")}
    sl = {n: t[:, 3:3 + K] for n, t in outs.items()}
    loss, loss2 = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    yv.ops.sigmoid_bce(zs, y.cuda(), loss, sl["dl"], sl["prob"])
    yv.ops.sigmoid(zs, sl["prob2"])
    yv.ops.bce(sl["prob2"], y.cuda(), loss2, sl["dp"])
    yv.ops.sigmoid_bwd(sl["dp"], sl["prob2"], sl["dl2"])
    for pn, dn, ls in (("prob", "dl", loss), ("prob2", "dl2", loss2)):
        close(sl[pn], p64, msg=pn)
        close(sl[dn], dz64, msg=dn)
        close(ls, loss64, msg="loss")
    for n, t in outs.items():
        assert bool((t[:, :3] == -7.0).all()) and bool((t[:, 3 + K:] == -7.0).all()), n
    assert bool((wide[:, :5] == 1e30).all()) and bool((wide[:, 5 + K:] == 1e30).all())


def test_saturation_quirk_matches_torch_fp32():
    """Where p rounds to exactly 1.0f / 0.0f, torch's BCELoss backward followed by its sigmoid backward gives a ZERO
    gradient and a wrong element costs exactly 100; at z = -30 with target 1 the 1e-12 clamp of the backward is active.
    Entries from {+-30, +-100} and |z| <= 4 only (16 < |z| < 18 and 87 < |z| < 90 are decided by the last bit of expf /
    fp32 denormals in the reference itself); labels chosen so that every combination occurs."""
    yv = _yv()
    K = 6
    sat = [30.0, -30.0, 100.0, -100.0]
    rows, labels = [], []
    g = torch.Generator().manual_seed(5)
    for v in sat:                       # the saturated entry in column c, the label on it (c == 2) or beside it
        for lab in (2, 3):
            r = (torch.rand(K, generator=g) * 8 - 4)
            r[2] = v
            rows.append(r)
            labels.append(lab)
    rows.append(torch.tensor([30.0, -30.0, 100.0, -100.0, 0.5, -0.5])); labels.append(1)     # clamp active: z = -30, t = 1
    rows.append(torch.tensor([100.0, 100.0, -100.0, -100.0, 30.0, -30.0])); labels.append(3)
    rows.append(torch.rand(K, generator=g) * 8 - 4); labels.append(0)                         # an ordinary row
    z = torch.stack(rows)
    y = torch.tensor(labels)
    az = z.abs()
    assert bool(((az <= 4) | (az == 30) | (az == 100)).all())
    p32, loss32, dz32 = _torch_ref(z, y, torch.float32)
    tgt = torch.zeros_like(z).scatter_(1, y.unsqueeze(1), 1)
    one, zero = p32 == 1.0, p32 == 0.0
    # every combination occurs in the reference: saturated and right / wrong on both sides, and the clamp
    assert bool((one & (tgt == 1)).any()) and bool((one & (tgt == 0)).any())
    assert bool((zero & (tgt == 1)).any()) and bool((zero & (tgt == 0)).any())
    q32 = p32 * (1 - p32)
    assert bool(((q32 < 1e-12) & (q32 > 0) & (tgt == 1)).any())
    for name, fn in (("fused", _fused), ("composed", _composed)):
        prob, loss, dl = fn(yv, z.cuda(), y.cuda())
        prob, dl = prob.cpu(), dl.cpu()
        assert torch.equal(prob == 1.0, one) and torch.equal(prob == 0.0, zero), name
        assert bool((dl[dz32 == 0] == 0).all()), name
        close(prob, p32, msg="%s prob" % name)
        close(loss, loss32, msg="%s loss" % name)
        close(dl, dz32, msg="%s dlogits" % name)
    # the loss term of a saturated, wrong element is 100: one such element in a row of otherwise exact zeros
    z1 = torch.full((1, 4), -100.0)
    z1[0, 1] = 100.0
    for lab, want in ((1, 0.0), (0, 200.0 / 4)):            # right: no loss at all; wrong: two elements at 100 each
        _, loss, dl = _fused(yv, z1.cuda(), torch.tensor([lab]).cuda())
        assert float(loss) == want and bool((dl == 0).all())


@pytest.mark.parametrize("bad", [-1, "K"])
def test_bad_label_poisons_the_loss_and_nothing_else(bad):
    yv = _yv()
    P, K = 257, 33
    z, y, p64, loss64, dz64 = _ref64(P, K)
    y = y.clone()
    y[100] = K if bad == "K" else -1
    for fn in (_fused, _composed):
        prob, loss, dl = fn(yv, z.cuda(), y.cuda())
        assert bool(torch.isnan(loss).all())
        dl = dl.cpu()
        keep = torch.arange(P) != 100
        assert bool(torch.isfinite(dl[keep]).all())
        close(dl[keep], dz64[keep], msg="dlogits of the other rows")


@pytest.mark.parametrize("P,K", [(257, 33), (3000, 22)])
def test_fused_equals_the_three_call_sequence_bitwise(P, K):
    yv = _yv()
    z, y = _draw(P, K)
    pf, lf, df = _fused(yv, z.cuda(), y.cuda())
    pc, lc, dc = _composed(yv, z.cuda(), y.cuda())
    assert torch.equal(lf, lc)
    assert torch.equal(df, dc)
    assert torch.equal(pf, pc)


def test_two_runs_are_bit_identical():
    yv = _yv()
    z, y = _draw(3000, 22)
    a = _fused(yv, z.cuda(), y.cuda())
    b = _fused(yv, z.cuda(), y.cuda())
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    in_place = z.cuda()
    assert yv.ops.sigmoid(in_place, in_place) is in_place and torch.equal(in_place, a[0])      # out may alias z
