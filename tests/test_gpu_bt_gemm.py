"""GPU tests (-m gpu) of the three GEMM forms of the bf16_dense training precision — yolat_bt_linear_fwd, _fwd_wt and
_bwd_w (csrc/bf16_train.hip) — against float64 products of the once-rounded operands (tests/head_ref.py).

Activations and gradients are k / 4096 (not bfloat16 values, ties of the rounding frequent), the prologue's (scale, shift)
lie on the exact grid of bf16_ref, so the reference bf(relu(a scale + shift)) has no rounding ambiguity.  Every operand
and output is a slot of a wider NaN-filled buffer (16-byte rows where bt_vec_ok asks for them), everything outside the
output stays NaN, each op runs twice with the same bits, and every element is held to
    dot_delta(|bf(pro(A))| . |bf(W)|^T + |bias|, K_red) + u |want|.
Each test prints `ratio <op> <tensor> <worst error / tolerance>`."""
import pytest
import torch

import bf16_ref as br
import head_ref as hr

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _ops():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv.ops


def _lib():
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    return lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _judge(op, name, got, want, tol):
    r, bad = hr.ratio(got, want, tol)
    print("ratio %-14s %-8s %.4f" % (op, name, r))
    assert bad == 0, "%s %s: %d elements outside the tolerance, worst error / tolerance %.3f" % (op, name, bad, r)
    return r


def _pro(kind, K, seed):
    """(scale, shift, relu) on the device in NaN-guarded vectors, or (None, None, False)"""
    if kind == "none":
        return None, None, False
    scale, shift = br.grid_scale_shift(K, seed)
    return hr.Vec(K, DEV).set(scale.to(DEV)), hr.Vec(K, DEV).set(shift.to(DEV)), kind == "relu"


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------
# Y = pro(A) . W^T + bias (+ BatchNorm partial statistics)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,pro,with_bias,with_stats", hr.BT_FWD_CASES)
def test_bt_linear_fwd_matches_fp64_per_element(M, K, N, pro, with_bias, with_stats):
    """k_bt_gemm<false, false>: M around the 32-row wave groups and the 64-row tile (1, 31, 33, 64, 65, 129, 300), N with
    column tails (1, 33, 65, 127, 72, 130), K from one LDS stage (32) to 72 (2304).  Statistics: (sum, M2) per 32-row group
    of the STORED values, the tail group with cnt = M % 32, nothing past 2 ceil(M / 32) N."""
    ops = _ops()
    seed = M + K + N
    A = hr.Slot(M, K, DEV, left=4, right=8)
    A.set(hr.bt_activation(M, K, seed).to(DEV))
    W = hr.Slot(N, K, DEV, left=8, right=4)
    W.set(hr.bt_weight(N, K, seed + 1).to(DEV))
    bias = hr.Vec(N, DEV).set(_randn((N,), seed + 2).to(DEV)) if with_bias else None
    scale, shift, relu = _pro(pro, K, seed + 3)
    if scale is not None:
        assert br.prologue_is_exact_in_fp32(A.view, scale, shift)
    Y = hr.Slot(M, N, DEV, left=3, right=2)
    assert A.ld > K and W.ld > K and Y.ld > N and A.view.data_ptr() % 16 == 0 and W.view.data_ptr() % 16 == 0

    def run():
        Y.clear()
        st = None
        if with_stats:
            st = ops.stats_buffer(M, N, DEV)
            st.fill_(NAN)
        ops.bt_linear_fwd(A.view, W.view, bias, Y.view, a_pro=None if scale is None else (scale, shift), a_relu=relu,
                          stats=st)
        torch.cuda.synchronize()
        assert Y.outside_is_nan(), "bt_linear_fwd wrote outside Y"
        return Y.view.clone(), st
    y1, st1 = run()
    y2, st2 = run()
    assert torch.equal(_bits(y1), _bits(y2))
    want, tol = hr.bt_gemm_ref(hr.bt_operand(A.view, scale, shift, relu), br.bf(W.view), K, bias=bias)
    _judge("bt_fwd", "Y", y1, want, tol)
    if with_stats:
        G = (M + 31) // 32
        n = 2 * G * N
        assert torch.equal(_bits(st1[:n]), _bits(st2[:n]))
        assert bool(torch.isnan(st1[n:]).all()), "statistics written past the last row group"
        got = st1[:n].view(G, N, 2)
        s, m2, ts, tm = hr.bt_stats_ref(y1.double())
        _judge("bt_fwd", "sum", got[:, :, 0], s, ts)
        _judge("bt_fwd", "M2", got[:, :, 1], m2, tm)


def test_bt_fwd_cases_cover_every_option():
    assert {c[3] for c in hr.BT_FWD_CASES} == {"none", "affine", "relu"}
    assert {c[4] for c in hr.BT_FWD_CASES} == {True, False} and {c[5] for c in hr.BT_FWD_CASES} == {True, False}


# ---------------------------------------------------------------------------------------------
# Y (+)= A . Wt
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,K,N", hr.BT_WT_CASES)
def test_bt_linear_fwd_wt_matches_fp64_per_element(M, K, N, accumulate):
    """k_bt_gemm<false, true>: the weight is read k-major ([K][N], 8 columns per thread), N % 64 in {8, 8, 8, 0}; the
    accumulating store adds one rounding of base + product"""
    ops = _ops()
    seed = M + K + N
    A = hr.Slot(M, K, DEV, left=4, right=8)
    A.set(hr.bt_activation(M, K, seed).to(DEV))
    Wt = hr.Slot(K, N, DEV, left=8, right=4)
    Wt.set(hr.bt_weight(K, N, seed + 1).to(DEV))
    base = _randn((M, N), seed + 2).to(DEV)
    Y = hr.Slot(M, N, DEV, left=3, right=2)
    outs = []
    for _ in range(2):
        Y.clear()
        if accumulate:
            Y.set(base)
        ops.bt_linear_fwd_wt(A.view, Wt.view, Y.view, accumulate=accumulate)
        torch.cuda.synchronize()
        assert Y.outside_is_nan(), "bt_linear_fwd_wt wrote outside Y"
        outs.append(Y.view.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    want, tol = hr.bt_gemm_ref(br.bf(A.view), br.bf(Wt.view).t(), K, base=base if accumulate else None)
    _judge("bt_fwd_wt", "acc" if accumulate else "Y", outs[0], want, tol)


# ---------------------------------------------------------------------------------------------
# dW = dY^T . pro(A), db = column sums of dY
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,pro,with_db,split", hr.BT_DW_CASES)
def test_bt_linear_bwd_w_matches_fp64_per_element(M, N, K, pro, with_db, split):
    """k_bt_gemm<true, true> (both operands k-major: tail tiles of the transposed loads at M % 32 != 0), direct store
    (one split) or split-K partials + k_bt_reduce, as the work-size query states: (257, 72, 40) two splits of 160 with
    a last one of 97 rows, (1007, 256, 512) four of 256 with a last one of 239, (8000, 128, 128) thirty-two.  dW is a
    slot with lddw > K in both forms.  K_red = M + splits."""
    ops, lib = _ops(), _lib()
    seed = M + K + N
    S, kper = hr.bt_dw_plan(M, N, K)
    work = int(lib.yolat_bt_linear_bwd_w_work_elems(M, N, K))
    direct = -(-M // 32) * N + 64
    assert work == hr.bt_dw_work_elems(M, N, K)
    assert (work > direct) == split and (S > 1) == split, "the plan does not take the %s path" % ("split-K" if split else "direct")
    if split:
        assert work - direct == S * N * K
    dY = hr.Slot(M, N, DEV, left=4, right=4)
    dY.set(hr.bt_activation(M, N, seed).to(DEV))
    A = hr.Slot(M, K, DEV, left=8, right=8)
    A.set(hr.bt_activation(M, K, seed + 1).to(DEV))
    scale, shift, relu = _pro(pro, K, seed + 3)
    if scale is not None:
        assert br.prologue_is_exact_in_fp32(A.view, scale, shift)
    dW = hr.Slot(N, K, DEV, left=3, right=2)
    db = hr.Vec(N, DEV) if with_db else None
    assert dW.ld > K
    outs = []
    for _ in range(2):
        dW.clear()
        if db is not None:
            db.clear()
        ops.bt_linear_bwd_w(dY.view, A.view, dW.view, db.view if db is not None else None,
                            a_pro=None if scale is None else (scale, shift), a_relu=relu)
        torch.cuda.synchronize()
        assert dW.outside_is_nan(), "bt_linear_bwd_w wrote outside dW"
        assert db is None or db.outside_is_nan(), "bt_linear_bwd_w wrote outside db"
        outs.append((dW.view.clone(), db.view.clone() if db is not None else None))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    want, tol = hr.bt_gemm_ref(br.bf(dY.view).t(), hr.bt_operand(A.view, scale, shift, relu).t(), M + S)
    _judge("bt_bwd_w", "dW/split" if split else "dW/direct", outs[0][0], want, tol)
    if db is not None:
        assert torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        wdb, tdb = hr.bt_db_ref(dY.view)
        _judge("bt_bwd_w", "db", outs[0][1], wdb, tdb)


def test_bt_bwd_w_cases_cover_both_paths_and_options():
    assert {c[5] for c in hr.BT_DW_CASES} == {True, False} and {c[4] for c in hr.BT_DW_CASES} == {True, False}
    assert {c[3] for c in hr.BT_DW_CASES} == {"none", "relu"}
    assert {c[0] for c in hr.BT_DW_CASES} == {1, 31, 33, 255, 257, 1007, 8000}


# ---------------------------------------------------------------------------------------------
# declines
# ---------------------------------------------------------------------------------------------
def test_bt_gemms_decline_what_they_do_not_take_and_write_nothing():
    """YOLAT_E_UNSUPPORTED surfaces as the wrappers' ValueError, the NaN-filled output is untouched"""
    ops = _ops()

    def slot(r, c, **kw):
        s = hr.Slot(r, c, DEV, **kw)
        s.set(_randn((r, c), r + c).to(DEV))
        return s
    W32, Wt32 = slot(16, 32, left=4, right=4), slot(32, 16, left=4, right=4)
    cases = []
    # K % 32 != 0 for fwd
    Y = hr.Slot(8, 16, DEV)
    cases.append((Y, lambda: ops.bt_linear_fwd(slot(8, 48).view, slot(16, 48).view, None, Y.view)))
    # N % 8 != 0 for fwd_wt
    Y2 = hr.Slot(8, 12, DEV)
    cases.append((Y2, lambda: ops.bt_linear_fwd_wt(slot(8, 32).view, slot(32, 12).view, Y2.view)))
    # K % 8 != 0 for bwd_w
    dW = hr.Slot(8, 12, DEV)
    cases.append((dW, lambda: ops.bt_linear_bwd_w(slot(40, 8).view, slot(40, 12).view, dW.view)))
    # lda % 4 != 0 (the base is aligned: row 2 of a 38-float pitch starts at float 80)
    A38 = slot(8, 32, left=4, right=2, ld=38)
    assert A38.view.data_ptr() % 16 == 0 and A38.view.stride(0) == 38
    Y3, Y4, dW2 = hr.Slot(8, 16, DEV), hr.Slot(8, 16, DEV), hr.Slot(16, 32, DEV)
    cases.append((Y3, lambda: ops.bt_linear_fwd(A38.view, W32.view, None, Y3.view)))
    cases.append((Y4, lambda: ops.bt_linear_fwd_wt(A38.view, Wt32.view, Y4.view)))
    cases.append((dW2, lambda: ops.bt_linear_bwd_w(slot(8, 16).view, A38.view, dW2.view)))
    # a base pointer 4 bytes off a 16-byte boundary, pitch a multiple of 4
    A5 = slot(8, 32, left=5, right=3)
    assert A5.view.data_ptr() % 16 == 4 and A5.view.stride(0) % 4 == 0
    Y5, Y6, dW3 = hr.Slot(8, 16, DEV), hr.Slot(8, 16, DEV), hr.Slot(32, 16, DEV)
    cases.append((Y5, lambda: ops.bt_linear_fwd(A5.view, W32.view, None, Y5.view)))
    cases.append((Y6, lambda: ops.bt_linear_fwd_wt(A5.view, Wt32.view, Y6.view)))
    cases.append((dW3, lambda: ops.bt_linear_bwd_w(A5.view, slot(8, 16).view, dW3.view)))
    for i, (out, call) in enumerate(cases):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert out.all_nan(), "declined call %d wrote its output" % i
