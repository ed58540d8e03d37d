"""GPU tests (-m gpu) of the ops that close a training step — yolat_softmax_ce, yolat_adam_step, yolat_dropout_fwd /
_bwd (csrc/loss_optim.hip) — against the float64 references and per-element envelopes of tests/head_ref.py.

Conventions (as in test_gpu_bf16_storage_ops.py): every device operand and output is a slot inside a larger NaN-filled
buffer with a leading dimension above its width; after the call everything outside the output slot is still NaN (a read
outside an input slot would poison the result, which must be finite and inside its bound); each op runs twice on fresh
outputs and returns the same bits; no tolerance is scaled by a tensor maximum.  Each test prints `ratio <op> <tensor>
<worst error / tolerance>`."""
import math

import numpy as np
import pytest
import torch

import bf16_ref as br
import head_ref as hr

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _lib():
    from yolat_vectorgraphicsrecognition_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _judge(op, name, got, want, tol, where=None):
    r, bad = hr.ratio(got, want, tol, where)
    print("ratio %-14s %-8s %.4f" % (op, name, r))
    assert bad == 0, "%s %s: %d elements outside the tolerance, worst error / tolerance %.3f" % (op, name, bad, r)
    return r


# ---------------------------------------------------------------------------------------------
# softmax cross entropy
# ---------------------------------------------------------------------------------------------
def _ce_call(z, y, work=True, want_dl=True):
    """One call of yolat_softmax_ce on slots.  Returns (rc, loss [1] fp32 cpu, dl [P,K] cpu or None)."""
    L = _lib()
    P, K = z.shape
    zs = hr.Slot(P, K, DEV, left=3, right=2)
    zs.set(z.to(DEV))
    lab = torch.full((P + 9,), 1 << 40, dtype=torch.int64, device=DEV)          # a guard label read poisons the loss
    lab[4:4 + P] = y.to(DEV)
    dls = hr.Slot(P, K, DEV, left=1, right=6)
    loss = hr.Vec(1, DEV, off=3)
    nwork = int(L.lib.yolat_softmax_ce_work_elems(P))
    assert nwork >= hr.ce_workgroups(P)
    wk = hr.Vec(nwork, DEV)
    rc = L.lib.yolat_softmax_ce(zs.view.data_ptr(), zs.ld, lab[4:].data_ptr(), P, K, loss.view.data_ptr(),
                                dls.view.data_ptr() if want_dl else None, dls.ld,
                                wk.view.data_ptr() if work else None, _stream())
    torch.cuda.synchronize()
    assert loss.outside_is_nan() and wk.outside_is_nan(), "softmax_ce wrote outside loss / scratch"
    if want_dl:
        assert dls.outside_is_nan(), "softmax_ce wrote outside the dlogits slot"
    else:
        assert dls.all_nan(), "softmax_ce wrote dlogits although it was NULL"
    if not work:
        assert wk.all_nan()
    return rc, loss.view.cpu().clone(), dls.view.cpu().clone() if want_dl else None


def _ce_check(z, y, work, tag):
    P, K = z.shape
    rows = hr.ce_rows_kernel(K, work)
    rc, l1, d1 = _ce_call(z, y, work)
    rc2, l2, d2 = _ce_call(z, y, work)
    assert rc == 0 and rc2 == 0
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(d1), _bits(d2)), "softmax_ce is not deterministic"
    rc3, l3, _ = _ce_call(z, y, work, want_dl=False)
    assert rc3 == 0 and torch.equal(_bits(l1), _bits(l3)), "dlogits = NULL changes the loss bits"
    ref = hr.softmax_ce_ref(z, y, rows)
    op = "softmax_ce" + ("/rows" if rows else "/single")
    _judge(op, "loss", l1[0], ref["loss"], ref["tol_loss"])
    _judge(op, "dl", d1, ref["dl"], ref["tol_dl"])
    return ref, l1, d1


@pytest.mark.parametrize("P,K", hr.CE_ROWS_SHAPES)
def test_softmax_ce_rows_kernel_matches_fp64(P, K):
    """k_softmax_ce_rows + k_ce_final: scratch given and K <= 32.  (262444, 5) has 1026 workgroups: the second trip of
    k_ce_final's stride loop."""
    assert K <= 32 and hr.ce_rows_kernel(K, True)
    if P > 262144:
        assert hr.ce_workgroups(P) > 1024
    z, y = hr.ce_inputs(P, K, "randn3", 100 + P + K)
    _ce_check(z, y, True, "rows")


@pytest.mark.parametrize("P,K,work", hr.CE_SINGLE_SHAPES)
def test_softmax_ce_single_workgroup_kernel_matches_fp64(P, K, work):
    """k_softmax_ce: K > 32 (257 rows: one trip of the 1024-thread row loop, 1025: two), or no scratch buffer"""
    assert K > 32 or not work
    assert not hr.ce_rows_kernel(K, work)
    z, y = hr.ce_inputs(P, K, "randn3", 100 + P + K)
    _ce_check(z, y, work, "single")


@pytest.mark.parametrize("family", hr.ce_families())
@pytest.mark.parametrize("P,K", hr.CE_FAMILY_SHAPES)
def test_softmax_ce_input_families(P, K, family):
    z, y = hr.ce_inputs(P, K, family, 7 + K)
    ref, loss, dl = _ce_check(z, y, True, family)
    if family == "sure50":
        assert float(dl[3, int(y[3])]) == 0.0, "p_y rounds to 1: the gradient of the label column is exactly 0"
    if family == "spread90":
        assert bool((dl == 0).any(1).all()), "an underflowed column has p exactly 0"
    if family == "equal":                    # every column that is not the label holds the same bits, fl(fl(1 / K) / P)
        off = dl.clone()
        rows = torch.arange(P)
        off[rows, y] = off[rows, (y + 1) % K]
        assert torch.equal(_bits(off), _bits(off[:, :1].expand(P, K)))


def test_softmax_ce_label_out_of_range_poisons_the_loss_only():
    P, K = 257, 17
    z, y = hr.ce_inputs(P, K, "randn3", 5)
    y[11], y[200] = -1, K
    ref = hr.softmax_ce_ref(z, y, True)
    for work in (True, False):
        rc, loss, dl = _ce_call(z, y, work)
        assert rc == 0 and math.isnan(float(loss[0]))
        _judge("softmax_ce/badlabel", "dl", dl, ref["dl"], ref["tol_dl"], ref["good"][:, None].expand_as(ref["dl"]))


# ---------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------
class _AdamState(object):
    """param / grad / m / v as views one float into NaN-guarded buffers"""

    def __init__(self, p, g, m, v):
        self.vecs = [hr.Vec(p.numel(), DEV, off=1) for _ in range(4)]
        for vec, t in zip(self.vecs, (p, g, m, v)):
            vec.set(t.to(DEV))

    def step(self, wd, gs, step):
        ops = _yv().ops
        p, g, m, v = [x.view for x in self.vecs]
        gbits = _bits(g).clone()
        ops.adam_step(p, g, m, v, hr.ADAM_HP["lr"], hr.ADAM_HP["beta1"], hr.ADAM_HP["beta2"], hr.ADAM_HP["eps"], wd, step,
                      grad_scale=gs)
        torch.cuda.synchronize()
        assert all(x.outside_is_nan() for x in self.vecs), "adam_step wrote into a guard element"
        assert torch.equal(_bits(g), gbits), "adam_step changed the gradient"
        return p.cpu().clone(), m.cpu().clone(), v.cpu().clone()


def _adam_one(state, cfg, tag):
    """one kernel step from `state` (cpu fp32 p, g, m, v), twice, judged against the float64 step from that state"""
    wd, gs, step = cfg
    out1 = _AdamState(*state).step(wd, gs, step)
    out2 = _AdamState(*state).step(wd, gs, step)
    for a, b in zip(out1, out2):
        assert torch.equal(_bits(a), _bits(b)), "adam_step is not deterministic"
    ref = hr.adam_ref(*state, wd=wd, step=step, grad_scale=gs, **hr.ADAM_HP)
    for name, got in zip("pmv", out1):
        _judge("adam", name, got, ref[name], ref["tol_" + name])
    return out1


ADAM_CASES = list(dict.fromkeys([(n, hr.ADAM_GRID[i % len(hr.ADAM_GRID)]) for i, n in enumerate(hr.ADAM_N)]
                                + [(n, c) for n in (257, 100003) for c in hr.ADAM_GRID]))


@pytest.mark.parametrize("n,cfg", ADAM_CASES)
def test_adam_step_matches_fp64_per_element(n, cfg):
    """one step; n = 4096 * 256 + 1 puts one element into the second trip of the grid-stride loop (4096 blocks of 256)"""
    wd, gs, step = cfg
    p, g, m, v, fam = hr.adam_inputs(n, n + step)
    pn, mn, vn = _adam_one((p, g, m, v), cfg, "n%d" % n)
    if wd == 0.0:
        z = fam == 1
        assert torch.equal(_bits(pn[z]), _bits(p[z])), "g = m = v = 0 must leave the parameter bit-identical"
        assert bool((mn[z] == 0).all()) and bool((vn[z] == 0).all())


def test_adam_grid_reaches_the_second_stride_trip():
    assert hr.ADAM_N[-1] > 4096 * 256 and any(n == hr.ADAM_N[-1] for n, _ in ADAM_CASES)
    assert {c for _, c in ADAM_CASES} == set(hr.ADAM_GRID)


def test_adam_chained_steps_each_judged_from_the_kernels_own_state():
    n = 257
    p, g, m, v, _ = hr.adam_inputs(n, 41)
    gen = torch.Generator().manual_seed(42)
    for step in (1, 2, 3):
        p, m, v = _adam_one((p, g, m, v), (1e-5, 1.0 / 3.0, step), "chain%d" % step)
        g = torch.randn(n, generator=gen)


def test_adam_five_steps_against_torch_adam_with_grad_scale():
    """Five chained steps at grad_scale = 0.125 (raw gradients for the kernel, pre-multiplied ones — exact, a power of two
    — for torch.optim.Adam in fp32 on the CPU), plain randn state.  Kernel and torch each stay within the step's envelope
    of the exact step from their own state; the step map does not expand m or v differences (factors beta1, beta2 < 1) and
    carries a p difference over unchanged, so after T steps |kernel - torch| <= 2 sum_t tol_t for m and v, and T times
    that for p (every earlier step's m and v difference enters the later updates at first order through the terms tol_p
    already holds)."""
    n, T, wd, gs = 4099, 5, 1e-5, 0.125
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=gen)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=hr.ADAM_HP["lr"], betas=(hr.ADAM_HP["beta1"], hr.ADAM_HP["beta2"]),
                           eps=hr.ADAM_HP["eps"], weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    acc = dict(p=torch.zeros(n, dtype=torch.float64), m=torch.zeros(n, dtype=torch.float64),
               v=torch.zeros(n, dtype=torch.float64))
    for step in range(1, T + 1):
        g = torch.randn(n, generator=gen) * 8
        ref = hr.adam_ref(p, g, m, v, wd=wd, step=step, grad_scale=gs, **hr.ADAM_HP)
        p, m, v = _AdamState(p, g, m, v).step(wd, gs, step)
        for k in acc:
            acc[k] += 2 * ref["tol_" + k]
        par.grad = g * gs
        opt.step()
    st = opt.state[par]
    _judge("adam/torch5", "p", p, par.detach().double(), T * acc["p"])
    _judge("adam/torch5", "m", m, st["exp_avg"].double(), acc["m"])
    _judge("adam/torch5", "v", v, st["exp_avg_sq"].double(), acc["v"])


# ---------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------
MASK_FILL = 0xAB


def _drop_fwd(Y, scale, shift, relu, p, seed):
    """yolat_dropout_fwd on slots; returns (rc, mask uint8 [M,C] numpy, Z fp32 [M,C] numpy, untouched)"""
    L = _lib()
    M, C = Y.shape
    ys, zs = hr.Slot(M, C, DEV, left=3, right=2), hr.Slot(M, C, DEV, left=2, right=7)
    ys.set(Y.to(DEV))
    mb = torch.full((M * C + 32,), MASK_FILL, dtype=torch.uint8, device=DEV)
    sc, sh = hr.Vec(C, DEV), hr.Vec(C, DEV)
    if scale is not None:
        sc.set(scale.to(DEV))
    if shift is not None:
        sh.set(shift.to(DEV))
    rc = L.lib.yolat_dropout_fwd(ys.view.data_ptr(), ys.ld, M, C, sc.view.data_ptr() if scale is not None else None,
                                 sh.view.data_ptr() if shift is not None else None, int(relu), float(p), int(seed),
                                 mb[16:].data_ptr(), zs.view.data_ptr(), zs.ld, _stream())
    torch.cuda.synchronize()
    guards_ok = bool((mb[:16] == MASK_FILL).all() and (mb[16 + M * C:] == MASK_FILL).all()) and zs.outside_is_nan()
    untouched = guards_ok and zs.all_nan() and bool((mb == MASK_FILL).all())
    assert guards_ok, "dropout_fwd wrote outside the mask / Z slot"
    return rc, mb[16:16 + M * C].cpu().numpy().reshape(M, C), zs.view.cpu().numpy(), untouched


PROLOGUES = [(False, False), (False, True), (True, False), (True, True)]          # (scale and shift, ReLU)


@pytest.mark.parametrize("p", hr.DROP_P)
@pytest.mark.parametrize("M,C", hr.DROP_SHAPES)
def test_dropout_fwd_mask_and_values_equal_the_documented_generator(M, C, p):
    seed = hr.DROP_SEEDS[0]
    Y = br.grid_activation(M, C, 3 + M).float()
    scale, shift = br.grid_scale_shift(C, 4 + C)
    assert br.prologue_is_exact_in_fp32(Y, scale, shift)
    for affine, relu in PROLOGUES:
        sc, sh = (scale, shift) if affine else (None, None)
        rc, mask, Z, _ = _drop_fwd(Y, sc, sh, relu, p, seed)
        rc2, mask2, Z2, _ = _drop_fwd(Y, sc, sh, relu, p, seed)
        assert rc == 0 and rc2 == 0
        assert np.array_equal(mask, mask2) and np.array_equal(Z.view(np.int32), Z2.view(np.int32))
        wmask, wZ = hr.dropout_fwd_ref(Y.numpy(), None if sc is None else sc.numpy(), None if sh is None else sh.numpy(),
                                       relu, p, seed)
        assert set(np.unique(mask)) <= {0, 1}
        assert np.array_equal(mask, wmask), "mask differs from the generator at %d positions" % int((mask != wmask).sum())
        assert np.array_equal(Z, wZ), "Z differs at %d positions" % int((Z != wZ).sum())
        assert (Z[mask == 0] == 0).all()
        if p == 0.0:
            assert mask.all() and np.array_equal(Z.view(np.int32), wZ.view(np.int32))
    if M * C == 1000 * 1024 and p > 0:
        assert hr.keep_count_ok(int(mask.sum()), M * C, p)


def test_dropout_threshold_edge_keeps_the_element_whose_hash_equals_it():
    """p chosen (head_ref.dropout_edge_p) so that p 2^32 equals the hash of one position: `>=` keeps it, `>` drops it"""
    M, C, seed = 333, 64, hr.DROP_SEEDS[0]
    p, idx = hr.dropout_edge_p(seed, M * C)
    Y = br.grid_activation(M, C, 5).float()
    rc, mask, Z, _ = _drop_fwd(Y, None, None, False, p, seed)
    assert rc == 0 and mask.reshape(-1)[idx] == 1
    wmask, wZ = hr.dropout_fwd_ref(Y.numpy(), None, None, False, p, seed)
    assert np.array_equal(mask, wmask) and np.array_equal(Z, wZ)
    assert not np.array_equal(mask, hr.dropout_mask(seed, M, C, p, defect="gt"))


def test_dropout_mask_is_a_function_of_seed_and_position_alone():
    """through ops.dropout_fwd: (333, 64) is the head of (400, 64) under one seed; another seed differs widely"""
    ops = _yv().ops
    seed = hr.DROP_SEEDS[1]

    def run(M, s):
        Y = br.grid_activation(M, 64, 6).float().to(DEV)
        Z = torch.full((M, 64), NAN, device=DEV)
        return ops.dropout_fwd(Y, None, None, False, 0.5, s, Z).cpu().numpy()
    a, b, c = run(333, seed), run(400, seed), run(333, seed + 1)
    assert a.shape == (333 * 64,) and np.array_equal(a, b[:333 * 64])
    assert np.array_equal(a, hr.dropout_mask(seed, 333, 64, 0.5).reshape(-1))
    assert (a != c).mean() > 0.25


@pytest.mark.parametrize("p", hr.DROP_P)
@pytest.mark.parametrize("M,C", hr.DROP_SHAPES)
def test_dropout_bwd_equals_dz_times_inv_keep_where_kept(M, C, p):
    ops = _yv().ops
    seed = hr.DROP_SEEDS[1]
    mask = hr.dropout_mask(seed, M, C, p)
    dZ = torch.randn(M, C, generator=torch.Generator().manual_seed(M + C))
    dzs, dxs = hr.Slot(M, C, DEV, left=1, right=4), hr.Slot(M, C, DEV, left=5, right=2)
    dzs.set(dZ.to(DEV))
    mb = torch.full((M * C + 32,), MASK_FILL, dtype=torch.uint8, device=DEV)
    mb[16:16 + M * C] = torch.from_numpy(mask.reshape(-1)).to(DEV)
    outs = []
    for _ in range(2):
        dxs.clear()
        ops.dropout_bwd(dzs.view, mb[16:16 + M * C], p, dxs.view)
        torch.cuda.synchronize()
        assert dxs.outside_is_nan()
        outs.append(dxs.view.cpu().numpy().copy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))
    want = hr.dropout_bwd_ref(dZ.numpy(), mask, p)
    assert np.array_equal(outs[0], want), "dX differs at %d positions" % int((outs[0] != want).sum())


def test_dropout_declines_and_empty_batch_write_nothing():
    yv, L = _yv(), _lib()
    Y = br.grid_activation(5, 7, 1).float()
    scale, shift = br.grid_scale_shift(7, 2)
    rc, _, _, untouched = _drop_fwd(Y[:0], None, None, False, 0.5, 1)                  # M = 0
    assert rc == 0 and untouched
    for kw in (dict(scale=None, shift=None, p=1.0), dict(scale=scale, shift=None, p=0.5),
               dict(scale=None, shift=None, p=float("nan")), dict(scale=None, shift=None, p=-0.1)):
        rc, _, _, untouched = _drop_fwd(Y, kw["scale"], kw["shift"], False, kw["p"], 1)
        assert rc == -1 and untouched, kw
    # the wrappers turn the code into their exception
    Yd = Y.to(DEV)
    Z = torch.full((5, 7), NAN, device=DEV)
    with pytest.raises(L.YolatLibraryError):
        yv.ops.dropout_fwd(Yd, None, None, False, 1.0, 1, Z)
    with pytest.raises(L.YolatLibraryError):
        yv.ops.dropout_fwd(Yd, scale.to(DEV), None, False, 0.5, 1, Z)
    dX = torch.full((5, 7), NAN, device=DEV)
    with pytest.raises(L.YolatLibraryError):
        yv.ops.dropout_bwd(Yd, torch.ones(35, dtype=torch.uint8, device=DEV), 1.0, dX)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Z).all()) and bool(torch.isnan(dX).all())
