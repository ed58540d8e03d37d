"""CPU tests of tests/head_ref.py: for every op of tests/test_gpu_head_ops.py and tests/test_gpu_bt_gemm.py the fp32
emulation written from the kernel source lies inside the float64 envelope at every shape and input family the GPU tests
use, every planted defect is rejected, and honest fp32 implementations from torch (cross_entropy, optim.Adam) lie inside
too — the envelopes are neither wider than a defect nor tighter than fp32 arithmetic."""
import math

import numpy as np
import pytest
import torch

import bf16_ref as br
import head_ref as hr


def _inside(got, want, tol, where=None):
    r, bad = hr.ratio(got, want, tol, where)
    return bad == 0, r


# ---------------------------------------------------------------------------------------------
# softmax cross entropy
# ---------------------------------------------------------------------------------------------
def _ce_judge(z, y, rows, loss, dl):
    ref = hr.softmax_ce_ref(z, y, rows)
    ok_l, r_l = _inside(torch.tensor(float(loss)), ref["loss"], ref["tol_loss"])
    ok_d, r_d = _inside(torch.from_numpy(np.asarray(dl)), ref["dl"], ref["tol_dl"], ref["good"][:, None].expand_as(ref["dl"]))
    return ok_l, ok_d, r_l, r_d


CE_ALL = [(P, K, True) for P, K in hr.CE_ROWS_SHAPES] + list(hr.CE_SINGLE_SHAPES)


@pytest.mark.parametrize("P,K,work", CE_ALL)
def test_softmax_ce_emulation_inside_envelope_at_every_shape(P, K, work):
    rows = hr.ce_rows_kernel(K, work)
    z, y = hr.ce_inputs(P, K, "randn3", 100 + P + K)
    loss, dl = hr.emulate_softmax_ce(z.numpy(), y.numpy(), rows)
    ok_l, ok_d, r_l, r_d = _ce_judge(z, y, rows, loss, dl)
    assert ok_l and ok_d, (r_l, r_d)


@pytest.mark.parametrize("family", hr.ce_families())
@pytest.mark.parametrize("P,K", hr.CE_FAMILY_SHAPES)
def test_softmax_ce_emulation_and_torch_inside_envelope_for_every_family(P, K, family):
    rows = hr.ce_rows_kernel(K, True)
    z, y = hr.ce_inputs(P, K, family, 7 + K)
    loss, dl = hr.emulate_softmax_ce(z.numpy(), y.numpy(), rows)
    ok_l, ok_d, r_l, r_d = _ce_judge(z, y, rows, loss, dl)
    assert ok_l and ok_d, (r_l, r_d)
    # an honest fp32 implementation: torch's cross_entropy and its autograd on the CPU
    zt = z.clone().requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(zt, y)
    lt.backward()
    ok_l, ok_d, r_l, r_d = _ce_judge(z, y, rows, lt.detach(), zt.grad.numpy())
    assert ok_l and ok_d, ("torch", r_l, r_d)


def test_softmax_ce_families_hold_what_they_are_for():
    f = np.float32
    for P, K in hr.CE_FAMILY_SHAPES:
        z, y = hr.ce_inputs(P, K, "spread90", 7 + K)
        e = np.exp((z.numpy() - z.numpy().max(1, keepdims=True)).astype(f))
        assert (e == 0).any(1).all(), "every row has an underflowed column"
        assert (e[np.arange(P), y.numpy()] == 0).sum() >= P // 2, "labels sit on underflowed columns"
        ref = hr.softmax_ce_ref(z, y, True)
        assert float(ref["loss"]) > 80.0
        z, y = hr.ce_inputs(P, K, "sure50", 7 + K)
        _, dl = hr.emulate_softmax_ce(z.numpy(), y.numpy(), hr.ce_rows_kernel(K, True))
        assert dl[3, int(y[3])] == 0.0, "p_y rounds to 1: the gradient is exactly 0"
        z, y = hr.ce_inputs(P, K, "offset1e4", 7 + K)
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(z.numpy())).all()


@pytest.mark.parametrize("defect,family,P,K,work", [
    ("inv_p1", "randn3", 257, 31, True), ("inv_p1", "randn3", 257, 33, True),
    ("no_max", "offset1e4", 257, 31, True), ("no_max", "offset1e4", 257, 33, True),
    ("wrong_row", "randn3", 257, 31, True), ("wrong_row", "randn3", 700, 17, False),
    ("drop_partial", "randn3", 257, 31, True), ("drop_partial", "randn3", 262144 + 300, 5, True),
    ("drop_partial", "randn3", 1025, 40, True)])
def test_softmax_ce_envelope_rejects_planted_defects(defect, family, P, K, work):
    rows = hr.ce_rows_kernel(K, work)
    z, y = hr.ce_inputs(P, K, family, 100 + P + K)
    loss, dl = hr.emulate_softmax_ce(z.numpy(), y.numpy(), rows, defect=defect)
    ok_l, ok_d, _, _ = _ce_judge(z, y, rows, loss, dl)
    assert not (ok_l and ok_d)
    if defect in ("wrong_row", "drop_partial"):
        assert not ok_l                       # these two touch the loss alone


def test_softmax_ce_bad_labels_poison_the_loss_only():
    P, K = 257, 17
    z, y = hr.ce_inputs(P, K, "randn3", 5)
    y[11], y[200] = -1, K
    ref = hr.softmax_ce_ref(z, y, True)
    assert math.isnan(float(ref["loss"])) and int(ref["good"].sum()) == P - 2
    loss, dl = hr.emulate_softmax_ce(z.numpy(), y.numpy(), True)
    assert math.isnan(float(loss))
    ok, r = _inside(torch.from_numpy(dl), ref["dl"], ref["tol_dl"], ref["good"][:, None].expand_as(ref["dl"]))
    assert ok, r


def test_ce_dispatch_and_depth():
    assert hr.ce_rows_kernel(32, True) and not hr.ce_rows_kernel(33, True) and not hr.ce_rows_kernel(17, False)
    assert hr.ce_workgroups(262144 + 300) == 1026                      # > 1024: the second trip of k_ce_final
    assert hr.ce_depth(262144 + 300, True) == 8 + 2 + 10 and hr.ce_depth(1025, False) == 2 + 10


# ---------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------
def _adam_judge(state, cfg, out):
    wd, gs, step = cfg
    ref = hr.adam_ref(*state, wd=wd, step=step, grad_scale=gs, **hr.ADAM_HP)
    res = {}
    for name, got in zip("pmv", out):
        res[name] = _inside(torch.from_numpy(np.asarray(got)), ref[name], ref["tol_" + name])
    return res


@pytest.mark.parametrize("cfg", hr.ADAM_GRID)
@pytest.mark.parametrize("n", hr.ADAM_N)
def test_adam_emulation_inside_envelope(n, cfg):
    wd, gs, step = cfg
    p, g, m, v, fam = hr.adam_inputs(n, n + step)
    out = hr.emulate_adam(p.numpy(), g.numpy(), m.numpy(), v.numpy(), wd=wd, step=step, grad_scale=gs, **hr.ADAM_HP)
    res = _adam_judge((p, g, m, v), cfg, out)
    assert all(ok for ok, _ in res.values()), res
    if wd == 0.0:                        # g = m = v = 0: the parameter comes back bit-identical
        z = (fam == 1).numpy()
        assert np.array_equal(out[0][z].view(np.int32), p.numpy()[z].view(np.int32))


def test_adam_grid_covers_every_value():
    assert {c[0] for c in hr.ADAM_GRID} == {0.0, 1e-5}
    assert {c[1] for c in hr.ADAM_GRID} == {1.0, 0.125, 1.0 / 3.0}
    assert {c[2] for c in hr.ADAM_GRID} == {1, 2, 1000, 10 ** 6}
    assert (1e-5, 1.0 / 3.0, 2) in hr.ADAM_GRID
    assert hr.ADAM_N[-1] > 4096 * 256                               # the grid-stride loop's second trip
    p, g, m, v, fam = hr.adam_inputs(100003, 3)
    f = np.float32
    with np.errstate(under="ignore"):
        assert (f(1e-30) * f(1e-30)) == 0.0                         # the tiny family's g^2 underflows
    assert bool((g[fam == 2].abs() == f(1e-30)).all()) and bool((g[fam == 3].abs() == f(1e15)).all())
    assert bool((p[fam == 4] == 0).all()) and bool((g[fam == 1] == 0).all())


@pytest.mark.parametrize("defect,cfg", [
    ("v_g", (0.0, 1.0, 1)), ("v_g", (1e-5, 1.0 / 3.0, 2)),
    ("eps_in_sqrt", (0.0, 1.0, 1)), ("eps_in_sqrt", (0.0, 0.125, 1000)),
    ("bc_step_m1", (1e-5, 1.0 / 3.0, 2)), ("bc_step_m1", (0.0, 0.125, 1000)),
    ("no_grad_scale", (0.0, 0.125, 1000)), ("no_grad_scale", (1e-5, 1.0 / 3.0, 2)),
    ("wd_always", (0.0, 1.0, 1)), ("wd_always", (0.0, 0.125, 1000))])
def test_adam_envelope_rejects_planted_defects(defect, cfg):
    wd, gs, step = cfg
    n = 100003
    p, g, m, v, _ = hr.adam_inputs(n, n + step)
    out = hr.emulate_adam(p.numpy(), g.numpy(), m.numpy(), v.numpy(), wd=wd, step=step, grad_scale=gs, defect=defect,
                          **hr.ADAM_HP)
    res = _adam_judge((p, g, m, v), cfg, out)
    assert not all(ok for ok, _ in res.values()), res


@pytest.mark.parametrize("wd,gs,step", [(0.0, 1.0, 1), (1e-5, 0.125, 1), (1e-5, 1.0, 7)])
def test_torch_adam_fp32_inside_envelope_for_one_step(wd, gs, step):
    """torch.optim.Adam in fp32 on the CPU, one step from a given state (gradient pre-multiplied by the power-of-two
    grad_scale, which is exact)"""
    n = 4099
    p, g, m, v, _ = hr.adam_inputs(n, 17)
    par = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([par], lr=hr.ADAM_HP["lr"], betas=(hr.ADAM_HP["beta1"], hr.ADAM_HP["beta2"]),
                           eps=hr.ADAM_HP["eps"], weight_decay=wd)
    par.grad = g * gs
    if step > 1:
        opt.state[par] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        state = (p, g, m, v)
    else:
        state = (p, g, torch.zeros(n), torch.zeros(n))
    opt.step()
    st = opt.state[par]
    res = _adam_judge(state, (wd, gs, step), (par.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()))
    assert all(ok for ok, _ in res.values()), res


# ---------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------
def test_hash32_is_the_splitmix64_finaliser():
    # splitmix64 seeded with 0: first outputs 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4 (the published test vector)
    h = hr.hash32(0, np.arange(2))
    assert int(h[0]) == 0xE220A839 and int(h[1]) == 0x6E789E6A
    assert hr.hash32((1 << 64) - 1, np.array([(1 << 63)], dtype=np.uint64)).dtype == np.uint32       # wraps, no error


def test_dropout_threshold_and_scale():
    assert hr.dropout_thresh(0.0) == 0 and hr.dropout_thresh(0.5) == 1 << 31
    assert hr.dropout_thresh(0.1) == int(float(np.float32(0.1)) * 2 ** 32)
    assert hr.dropout_thresh(float(np.nextafter(np.float32(1), np.float32(0)))) == (1 << 32) - 256
    assert hr.dropout_inv_keep(0.5) == 2.0 and hr.dropout_inv_keep(0.0) == 1.0
    assert bool(hr.dropout_mask(5, 40, 33, 0.0).all())                                 # p = 0 keeps everything


@pytest.mark.parametrize("seed", hr.DROP_SEEDS)
def test_dropout_generator_keep_rate_geometry_and_seeds(seed):
    n = 1000 * 1024
    for p in hr.DROP_P[1:]:
        assert hr.keep_count_ok(int(hr.dropout_mask(seed, 1000, 1024, p).sum()), n, p), p
    a = hr.dropout_mask(seed, 333, 64, 0.5).reshape(-1)
    b = hr.dropout_mask(seed, 400, 64, 0.5).reshape(-1)
    assert np.array_equal(a, b[:333 * 64])                       # a function of (seed, position) alone
    c = hr.dropout_mask(seed + 1, 333, 64, 0.5).reshape(-1)
    assert (a != c).mean() > 0.25


@pytest.mark.parametrize("M,C", hr.DROP_SHAPES[:3])
def test_dropout_reference_rejects_planted_defects(M, C):
    seed = hr.DROP_SEEDS[0]
    Y = br.grid_activation(M, C, 3).float()
    scale, shift = br.grid_scale_shift(C, 4)
    assert br.prologue_is_exact_in_fp32(Y, scale, shift)
    for p in hr.DROP_P:
        mask, Z = hr.dropout_fwd_ref(Y.numpy(), scale.numpy(), shift.numpy(), True, p, seed)
        assert set(np.unique(mask)) <= {0, 1}
        assert np.array_equal(Z != 0, (mask != 0) & (Z != 0)) and (Z[mask == 0] == 0).all()
        if p == 0.0:
            v = torch.relu(Y * scale + shift).numpy()
            assert np.array_equal(Z.view(np.int32), v.view(np.int32))
        if p > 0 and M * C > 64:
            for defect in ("transposed", "scale_dropped"):
                m2, Z2 = hr.dropout_fwd_ref(Y.numpy(), scale.numpy(), shift.numpy(), True, p, seed, defect=defect)
                assert not (np.array_equal(m2, mask) and np.array_equal(Z2, Z)), (defect, p)
    if M * C >= 333 * 64:
        # `>` instead of `>=` shows on the one element whose hash EQUALS the threshold: p chosen so that one exists
        p, idx = hr.dropout_edge_p(seed, M * C)
        assert 0.5 <= p < 0.95
        mask = hr.dropout_mask(seed, M, C, p).reshape(-1)
        wrong = hr.dropout_mask(seed, M, C, p, defect="gt").reshape(-1)
        assert mask[idx] == 1 and wrong[idx] == 0 and int((mask != wrong).sum()) >= 1


def test_dropout_bwd_ref():
    mask = hr.dropout_mask(9, 5, 7, 0.5)
    dZ = np.arange(35, dtype=np.float32).reshape(5, 7) + 1
    dX = hr.dropout_bwd_ref(dZ, mask.reshape(-1), 0.5)
    assert np.array_equal(dX, np.where(mask != 0, dZ * 2, 0))


# ---------------------------------------------------------------------------------------------
# bf16_dense GEMMs
# ---------------------------------------------------------------------------------------------
def _pro(kind, K, seed):
    if kind == "none":
        return None, None, False
    scale, shift = br.grid_scale_shift(K, seed)
    return scale, shift, kind == "relu"


def test_bt_inputs_are_what_the_envelope_assumes():
    A = hr.bt_activation(300, 512, 1)
    scale, shift = br.grid_scale_shift(512, 2)
    assert br.prologue_is_exact_in_fp32(A, scale, shift)
    assert float(A.abs().max()) <= 4.0
    rounded = A.to(torch.bfloat16).float()
    assert float((rounded != A).float().mean()) > 0.9                  # not bfloat16 values
    half = br.ulp_bf16(A).float() / 2
    ties = ((A - hr._round_bf16(A, "trunc")).abs() == half) & (A != 0)
    assert float(ties.float().mean()) > 1e-3                           # exact ties are frequent
    differ = hr._round_bf16(A, "away") != rounded
    assert bool((differ <= ties).all()) and int(differ.sum()) > 0      # ties away from zero differs on ties alone


@pytest.mark.parametrize("M,K,N,pro,with_bias,with_stats", hr.BT_FWD_CASES)
def test_bt_fwd_emulation_inside_envelope_and_defects_rejected(M, K, N, pro, with_bias, with_stats):
    seed = M + K + N
    A, W = hr.bt_activation(M, K, seed), hr.bt_weight(N, K, seed + 1)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)) if with_bias else None
    scale, shift, relu = _pro(pro, K, seed + 3)
    want, tol = hr.bt_gemm_ref(hr.bt_operand(A, scale, shift, relu), br.bf(W), K, bias=bias)
    wr = hr.emulate_bt_operand(W, None, None, False)
    got = hr.emulate_bt_gemm(hr.emulate_bt_operand(A, scale, shift, relu), wr, bias)
    ok, r = _inside(got, want, tol)
    assert ok, r
    s, m2, ts, tm = hr.bt_stats_ref(got.double())
    G = -(-M // 32)
    yp = torch.cat([got, torch.zeros(G * 32 - M, N)]).view(G, 32, N)
    cnt = torch.tensor([min(32, M - 32 * g) for g in range(G)], dtype=torch.float32).view(G, 1)
    s32 = yp.sum(1)
    d = (yp - (s32 / cnt)[:, None, :]) * (torch.arange(G * 32).view(G, 32, 1) < M)
    assert _inside(s32, s, ts)[0] and _inside((d * d).sum(1), m2, tm)[0]
    if M * N >= 64:
        assert not _inside(s32 * (1 + 2.0 ** -12), s, ts)[0]
    if M < 2:
        return
    # ties away from zero moves one operand in ~256 by a bfloat16 spacing, an error that grows like sqrt(K) under a
    # bound that grows like K: it is asked for at K <= 128, truncation (a bias, growing like K) everywhere
    for kw in (dict(mode="trunc"), dict(mode="away")):
        if kw["mode"] == "away" and K > 128:
            continue
        bad = hr.emulate_bt_gemm(hr.emulate_bt_operand(A, scale, shift, relu, **kw), wr, bias)
        assert not _inside(bad, want, tol)[0], kw
    assert not _inside(hr.emulate_bt_gemm(hr.emulate_bt_operand(A, scale, shift, relu), wr, bias, dup_last_row=True),
                       want, tol)[0]
    assert not _inside(hr.emulate_bt_gemm(hr.emulate_bt_operand(A, scale, shift, relu), wr, bias, skip_last_tile=True),
                       want, tol)[0]
    if scale is not None:
        bad = hr.emulate_bt_gemm(hr.emulate_bt_operand(A, scale, shift, relu, pro_after_round=True), wr, bias)
        assert not _inside(bad, want, tol)[0]


@pytest.mark.parametrize("M,K,N", hr.BT_WT_CASES)
def test_bt_fwd_wt_emulation_inside_envelope(M, K, N):
    seed = M + K + N
    A, Wt = hr.bt_activation(M, K, seed), hr.bt_weight(K, N, seed + 1)
    base = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 2))
    ar, wr = hr.emulate_bt_operand(A, None, None, False), hr.emulate_bt_operand(Wt, None, None, False)
    for b in (None, base):
        want, tol = hr.bt_gemm_ref(br.bf(A), br.bf(Wt).t(), K, base=b)
        got = hr.emulate_bt_gemm(ar, wr.t().contiguous())
        got = got if b is None else b + got
        ok, r = _inside(got, want, tol)
        assert ok, r
        if M >= 2:
            bad = hr.emulate_bt_gemm(hr.emulate_bt_operand(A, None, None, False, mode="trunc"), wr.t().contiguous())
            assert not _inside(bad if b is None else b + bad, want, tol)[0]


@pytest.mark.parametrize("M,N,K,pro,with_db,split", hr.BT_DW_CASES)
def test_bt_bwd_w_emulation_inside_envelope_and_defects_rejected(M, N, K, pro, with_db, split):
    seed = M + K + N
    S, kper = hr.bt_dw_plan(M, N, K)
    assert (S > 1) == split and kper % 32 == 0
    assert hr.bt_dw_work_elems(M, N, K) == (S * N * K if S > 1 else 0) + -(-M // 32) * N + 64
    dY, A = hr.bt_activation(M, N, seed), hr.bt_activation(M, K, seed + 1)
    scale, shift, relu = _pro(pro, K, seed + 3)
    want, tol = hr.bt_gemm_ref(br.bf(dY).t(), hr.bt_operand(A, scale, shift, relu).t(), M + S)
    dr = hr.emulate_bt_operand(dY, None, None, False).t().contiguous()
    ar = hr.emulate_bt_operand(A, scale, shift, relu).t().contiguous()
    splits = hr.bt_splits(M, N, K)
    got = hr.emulate_bt_gemm(dr, ar, splits=splits)
    ok, r = _inside(got, want, tol)
    assert ok, r
    db, tdb = hr.bt_db_ref(dY)
    assert _inside(dY.sum(0), db, tdb)[0]
    if M >= 33:
        assert not _inside(hr.emulate_bt_gemm(dr, ar, splits=splits, skip_last_tile=True), want, tol)[0]
        # a wrong rounding of operands of either sign adds up like sqrt(M) under a bound that grows like M (see the
        # forward): it is asked for where the reduction is short
        for mode in ("trunc", "away") if M <= 257 else ():
            bad = hr.emulate_bt_operand(A, scale, shift, relu, mode=mode).t().contiguous()
            assert not _inside(hr.emulate_bt_gemm(dr, bad, splits=splits), want, tol)[0], mode
        assert not _inside(hr.emulate_bt_gemm(dr, ar, splits=splits, dup_last_row=True), want, tol)[0]


def test_bt_dw_plans_named_in_the_cases():
    assert hr.bt_dw_plan(257, 72, 40) == (2, 160)                      # last split: 97 rows = 3 k tiles + 1 row
    assert hr.bt_dw_plan(1007, 256, 512) == (4, 256)                   # last split: 239 rows
    assert hr.bt_dw_plan(8000, 128, 128) == (32, 256)                  # 32 splits, the last of 64 rows
    assert hr.bt_dw_plan(255, 72, 40)[0] == 1
    assert {c[0] for c in hr.BT_DW_CASES} == {1, 31, 33, 255, 257, 1007, 8000}
