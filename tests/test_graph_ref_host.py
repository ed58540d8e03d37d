"""The helpers of tests/graph_ref.py are what they claim to be (no GPU needed): the ladder graph and the segment ladder,
the full-mantissa inputs and their ReLU-kink share, the float64 references against autograd, and — the proof that the GPU
tests of tests/test_gpu_fp32_graph_ops.py can fail for a subtly wrong kernel — every envelope accepts the defect-free
fp32 emulation on every graph used there and rejects each planted defect on the ladder and hub graphs."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import graph_ref as gr

pytestmark = pytest.mark.host

F32 = np.float32
HUBS_AND_LADDER = ["ladder", "hub65", "hub150", "hub1000"]


def _inside(got, want, tol):
    """(all inside, worst |err| / tol); NaN counts as outside"""
    got = torch.as_tensor(np.asarray(got)).double() if not torch.is_tensor(got) else got.double()
    err = (got - want).abs()
    ok = err <= tol
    r = err / tol.clamp_min(1e-300)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return bool(ok.all()), (float(r.max()) if r.numel() else 0.0)


def _csr_case(graph):
    """(N, E, d, s CSR-ordered int64 tensors, row_ptr, col_ptr, slots numpy) of a graph of the GPU tests"""
    N, src, dst = gr.GRAPHS[graph]()
    order, row_ptr, col_ptr, slots = gr.csr_of(src, dst, N)
    return N, len(src), torch.from_numpy(dst[order]), torch.from_numpy(src[order]), row_ptr, col_ptr, slots


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
def test_ladder_has_every_in_and_out_degree_once():
    src, dst = gr.ladder(seed=6)
    assert src.dtype == dst.dtype == np.int64 and len(src) == len(dst) == 820
    din, dout = np.bincount(dst, minlength=45), np.bincount(src, minlength=45)
    assert din[:41].tolist() == list(range(41)) and dout[:41].tolist() == list(range(41))
    assert not din[41:].any() and not dout[41:].any()
    assert 45 % 4 != 0 and 45 % 16 != 0
    assert {(int(n) // 8, int(n) % 8) for n in din[:41]} >= {(k, t) for k in range(5) for t in range(8)} | {(5, 0)}
    assert (np.diff(dst) < 0).any()                                   # the edge order is shuffled
    a, b = gr.ladder(seed=6)
    assert np.array_equal(a, src) and np.array_equal(b, dst)          # seeded
    c, _ = gr.ladder(seed=7)
    assert not np.array_equal(c, src)
    with pytest.raises(ValueError):
        gr.ladder(n_max=40, N=40)


@pytest.mark.parametrize("seed", range(8))
def test_segment_ladder_sizes(seed):
    sizes = gr.segment_ladder(seed)
    assert sizes.dtype == np.int64 and sorted(sizes.tolist()) == list(range(41)) + [300]
    assert sizes[0] > 0 and sizes[-1] > 0
    bb, ptr = gr.segment_ids(sizes)
    assert len(bb) == 820 + 300 and (np.diff(bb) >= 0).all() and ptr[-1] == len(bb)
    assert np.array_equal(np.bincount(bb, minlength=len(sizes)), sizes)
    big = int(np.argmax(sizes))
    assert (ptr[big + 1] - ptr[big]) // 8 == 37 and (ptr[big + 1] - ptr[big]) % 8 == 4   # 37 trips and a 4-row tail


def test_csr_of_is_the_stable_sort_and_the_csc_over_its_slots():
    N, src, dst = gr.GRAPHS["ladder"]()
    order, row_ptr, col_ptr, slots = gr.csr_of(src, dst, N)
    d, s = dst[order], src[order]
    assert (np.diff(d) >= 0).all() and row_ptr[-1] == col_ptr[-1] == len(src)
    for n in range(N):
        assert (d[row_ptr[n]:row_ptr[n + 1]] == n).all()
        sl = slots[col_ptr[n]:col_ptr[n + 1]]
        assert (s[sl] == n).all() and (np.diff(sl) > 0).all()


def test_inputs_carry_full_mantissas():
    inp = gr.bn_csr_inputs(300, 1000, 7)
    for k in ("Y", "A", "d_out", "W", "scale", "shift", "a_scale", "a_shift"):
        assert inp[k].dtype == torch.float32 and gr.has_full_mantissa(inp[k]), k
    assert gr.has_full_mantissa(gr.randn32((500, 64), 1))
    import bf16_ref as br
    assert not gr.has_full_mantissa(br.bn_bwd_inputs(300, 64, 1)[0].float())       # the bfloat16 generator: none


@pytest.mark.parametrize("N,E,kind", gr.BN_CSR_CASES + [(4000, 32832, "uniform")])
def test_bn_csr_inputs_stay_off_the_kink_and_their_fp32_masks_are_exact(N, E, kind):
    """the condition the envelopes of the statistics and of dY state: at most KINK_SHARE of the elements of Y (the
    BatchNorm behind the aggregation) within KINK of the ReLU kink — for every case of the GPU test, the three sizes
    32769, 32832 and 65537 at which the bfloat16 generator was checked among them.  And what lets the next BatchNorm's
    bound go without a kink term: the correctly rounded fp32 mask of either prologue IS the float64 mask."""
    inp = gr.bn_csr_inputs(N, E, 5 * N + E)
    assert gr.kink_share(inp["Y"], inp["scale"], inp["shift"]) <= gr.KINK_SHARE
    assert gr.relu_mask_is_exact(inp["A"], inp["a_scale"], inp["a_shift"])
    assert gr.relu_mask_is_exact(inp["Y"], inp["scale"], inp["shift"])
    if E >= 1000:
        y = inp["Y"].double()
        assert torch.allclose(inp["mean"].double(), y.mean(0), rtol=1e-6, atol=1e-7)
        assert torch.allclose(inp["invstd"].double(), 1 / torch.sqrt(y.var(0, unbiased=False) + 1e-5), rtol=1e-6)


@pytest.mark.parametrize("N,E,kind", gr.BN_CSR_MULTI_TILE)
def test_the_bfloat16_generator_stays_off_the_kink_at_the_multi_tile_cases(N, E, kind):
    """the two cases this file's cases share with test_gpu_bf16_storage_ops.py::BN_CSR_CASES, with that file's generator and seed"""
    import bf16_ref as br
    Y, _, mean, invstd, scale, shift = br.bn_bwd_inputs(E, 64, 5 * N + E)
    assert br.kink_share(Y, scale, shift) <= br.KINK_SHARE


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(3000).astype(F32)
    b = rng.standard_normal(3000).astype(F32)
    c = (rng.standard_normal(3000) * 10.0 ** rng.integers(-9, 3, 3000)).astype(F32)
    # double rounding: p = 2^-24 - 2^-70 is exact in float64, p + c is not, and the float64 sum lands exactly on an fp32
    # tie — with c = 1 + 2^-23 the tie's even neighbour is the WRONG one (the true sum lies below the tie), with c = 1 the
    # right one
    a = np.concatenate([a, F32([2.0 ** -24 * (1 + 2.0 ** -23)] * 2)])
    b = np.concatenate([b, F32([1 - 2.0 ** -23] * 2)])
    c = np.concatenate([c, F32([1 + 2.0 ** -23, 1.0])])
    assert float(np.float64(a[-1]) * np.float64(b[-1]) + np.float64(c[-2])) == 1 + 2.0 ** -23 + 2.0 ** -24   # the tie
    got = gr.fma32(a, b, c)
    assert got.dtype == F32

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = F32(float(v))                                              # a neighbour (float(v) rounds to float64 first)
        cands = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
        best = min(cands, key=lambda t: (abs(Fraction(float(t)) - v), int(t.view(np.uint32)) & 1))
        return best
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert float(got[-2]) == 1 + 2.0 ** -23 and float(got[-1]) == 1.0


# ---------------------------------------------------------------------------------------------
# references against autograd
# ---------------------------------------------------------------------------------------------
def test_mean_aggregation_reference_is_the_autograd_of_the_scatter_mean():
    N, E, d, s, *_ = _csr_case("hub150")
    C = 8
    h = gr.randn32((E, C), 1).double().requires_grad_(True)
    sc, sh = gr.pro_scale_shift(C, 2)
    d_out = gr.randn32((N, C), 3).double()
    want, tol, deg = gr.csr_mean_fwd_ref(h, sc, sh, True, d, N)
    t = torch.relu(h * sc.double() + sh.double())
    direct = torch.zeros(N, C, dtype=torch.float64).index_add(0, d, t) / torch.bincount(d, minlength=N).clamp_min(1)[:, None]
    assert torch.allclose(want, direct, rtol=1e-14, atol=0)
    assert torch.equal(deg.long(), torch.from_numpy(gr.in_degree(d.numpy(), N)))
    assert bool((tol[deg == 0] == 0).all()) and bool((tol[deg > 0] > 0).all())
    want.backward(d_out)
    mask = (h.detach() * sc.double() + sh.double() > 0).double()
    assert torch.allclose(h.grad, gr.csr_mean_bwd_ref(d_out, d, N) * mask * sc.double(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_mean_backward_envelope_accepts_the_fp32_arithmetic(graph, C):
    """d_out[dst] * fl(1 / max(deg, 1)) in fp32 lies within 2 u |q| of the float64 quotient, on every graph and with the
    operands of the GPU test"""
    N, E, d, s, *_ = _csr_case(graph)
    d_out = gr.randn32((N, C), N + E + C + 9)
    q = gr.csr_mean_bwd_ref(d_out, d, N)
    ok, worst = _inside(gr.csr_mean_bwd_fp32(d_out, d, N), q, 2.0 * gr.U * q.abs())
    assert ok and worst <= 1.0, worst
    # a kernel that divides by deg + 1 is outside
    deg = torch.bincount(d, minlength=N).clamp_min(1).double()
    assert not _inside(d_out.double()[d] / (deg[d][:, None] + 1), q, 2.0 * gr.U * q.abs())[0]


def test_bn_csr_references_are_the_autograd_of_linear_batchnorm_relu_mean():
    """dW, db, dA of bn_csr_consumers_ref, dY of bn_csr_dy_ref, dgamma / dbeta of bn_csr_stats_ref: autograd of
    out = scatter_mean(relu(batch_norm(relu(A a_scale + a_shift) . W^T + b))) in float64"""
    N, E, d, s, *_ = _csr_case("hub150")
    C = 64
    inp = gr.bn_csr_inputs(N, E, 11)
    A1 = torch.relu(inp["A"].double() * inp["a_scale"].double() + inp["a_shift"].double()).requires_grad_(True)
    W = inp["W"].double().requires_grad_(True)
    b = gr.randn32((C,), 12).double().requires_grad_(True)
    gamma = (torch.rand(C, generator=torch.Generator().manual_seed(13)).double() + 0.5).requires_grad_(True)
    beta = gr.randn32((C,), 14, 0.3).double().requires_grad_(True)
    Y = A1 @ W.t() + b
    Y.retain_grad()
    z = torch.relu(torch.nn.functional.batch_norm(Y, None, None, gamma, beta, True, 0.0, 1e-5))
    out = torch.zeros(N, C, dtype=torch.float64).index_add(0, d, z) / torch.bincount(d, minlength=N).clamp_min(1)[:, None]
    d_out = inp["d_out"].double()
    out.backward(d_out)
    y = Y.detach()
    mean, invstd = y.mean(0), 1 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)
    scale, shift = gamma.detach() * invstd, beta.detach() - mean * gamma.detach() * invstd
    ref, g0, tol_b, tol_g = gr.bn_csr_stats_ref(d_out, d, N, y, mean, invstd, scale, shift)
    assert torch.allclose(ref["dgamma"], gamma.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref["dbeta"], beta.grad, rtol=1e-10, atol=1e-12)
    dY, d_dY = gr.bn_csr_dy_ref(g0, y, mean, invstd, scale, shift, torch.cat([ref["c1"], ref["c2"]]))
    assert torch.allclose(dY, Y.grad, rtol=1e-9, atol=1e-13)
    con = gr.bn_csr_consumers_ref(dY, d_dY, A1.detach(), None, None, False, W.detach())
    assert torch.allclose(con["dW"], W.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(con["db"], b.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(con["dA"], A1.grad, rtol=1e-9, atol=1e-13)
    assert bool((con["tol_dW"] > 0).all() and (con["tol_db"] > 0).all() and (con["tol_dA"] > 0).all())


# ---------------------------------------------------------------------------------------------
# run sums: the envelopes accept the emulation, everywhere; and reject each defect on the ladder and the hubs
# ---------------------------------------------------------------------------------------------
def _mean_fwd(graph, mode, C, defect=None, mean_defect=None):
    N, E, d, s, row_ptr, _, _ = _csr_case(graph)
    pro, acc = mode.startswith("pro"), mode.endswith("acc")
    H = gr.randn32((E, C), N + E)
    sc, sh = gr.pro_scale_shift(C, N + E + 1) if pro else (None, None)
    base = gr.randn32((N, C), N + E + 2, 1.0, 3.0)
    sums = gr.emulate_run_sum(H.numpy(), row_ptr, trip=8, scale=None if not pro else sc.numpy(),
                              shift=None if not pro else sh.numpy(), relu=pro, defect=defect)
    got = gr.emulate_mean(sums, row_ptr, defect=mean_defect)
    if acc:
        got = got + base.numpy()
    want, tol, deg = gr.csr_mean_fwd_ref(H, sc, sh, pro, d, N, base if acc else None)
    return got, want, tol, deg, base


@pytest.mark.parametrize("mode", ["plain", "pro", "acc", "pro_acc"])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_mean_envelope_accepts_the_emulation(graph, mode):
    got, want, tol, deg, base = _mean_fwd(graph, mode, 20)
    ok, worst = _inside(got, want, tol)
    assert ok, worst
    empty = (deg == 0).numpy()
    if mode.endswith("acc"):
        assert np.array_equal(got[empty], base.numpy()[empty])
    else:
        assert (got[empty] == 0).all()


@pytest.mark.parametrize("defect", gr.RUN_DEFECTS + ("deg_divisor",))
@pytest.mark.parametrize("graph", HUBS_AND_LADDER)
def test_mean_envelope_rejects_every_defect(graph, defect):
    for mode in ("plain", "pro_acc"):
        if defect == "deg_divisor":
            got, want, tol, deg, _ = _mean_fwd(graph, mode, 20, mean_defect=defect)
            assert bool((deg == 0).any())
            bad = ~((torch.from_numpy(got).double() - want).abs() <= tol)
            assert bool(bad[deg == 0].all()) and not bool(bad[deg > 0].any())      # every empty node, nothing else
        else:
            got, want, tol, deg, _ = _mean_fwd(graph, mode, 20, defect=defect)
            ok, worst = _inside(got, want, tol)
            assert not ok and worst > 100.0, worst


def _scatter(graph, Cin, acc, defect=None):
    N, E, d, s, row_ptr, col_ptr, slots = _csr_case(graph)
    dG = gr.randn32((E, 2 * Cin), N + E + 5)
    base = gr.randn32((N, Cin), N + E + 6, 1.0, 3.0)
    g = dG.numpy()
    first = gr.emulate_run_sum(g[:, :Cin], row_ptr, trip=4, clamped=True, defect=defect)
    got = gr.emulate_run_sum(g[slots][:, Cin:], col_ptr, trip=4, clamped=True, init=first, defect=defect)
    if acc:
        got = got + base.numpy()
    want, tol = gr.edge_scatter_bwd_ref(dG, Cin, s, d, N, base if acc else None)
    return got, want, tol


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_scatter_envelope_accepts_the_emulation(graph, acc):
    for Cin in (5, 20):
        ok, worst = _inside(*_scatter(graph, Cin, acc))
        assert ok, worst


@pytest.mark.parametrize("defect", gr.RUN_DEFECTS)
@pytest.mark.parametrize("graph", HUBS_AND_LADDER)
def test_scatter_envelope_rejects_every_defect(graph, defect):
    for acc in (False, True):
        ok, worst = _inside(*_scatter(graph, 20, acc, defect))
        assert not ok and worst > 100.0, worst


def _uv_sums(graph, defect=None):
    N, E, d, s, row_ptr, col_ptr, slots = _csr_case(graph)
    dH = gr.randn32((E, 20), N + E + 7)
    h = dH.numpy()
    gu = gr.emulate_run_sum(h, row_ptr, trip=8, defect=defect)
    gv = gr.emulate_run_sum(h[slots], col_ptr, trip=8, clamped=True, defect=defect)
    return (gu, gv) + gr.edge_uv_sums_ref(dH, s, d, N)


@pytest.mark.parametrize("graph", sorted(gr.GRAPHS))
def test_uv_sums_envelope_accepts_the_emulation(graph):
    gu, gv, wu, tu, wv, tv = _uv_sums(graph)
    assert _inside(gu, wu, tu)[0] and _inside(gv, wv, tv)[0]


@pytest.mark.parametrize("defect", gr.RUN_DEFECTS)
@pytest.mark.parametrize("graph", HUBS_AND_LADDER)
def test_uv_sums_envelope_rejects_every_defect(graph, defect):
    gu, gv, wu, tu, wv, tv = _uv_sums(graph, defect)
    for got, want, tol in ((gu, wu, tu), (gv, wv, tv)):
        ok, worst = _inside(got, want, tol)
        assert not ok and worst > 100.0, worst


def _segment_mean(pro, defect=None, mean_defect=None, D=20):
    sizes = gr.segment_ladder()
    bb, ptr = gr.segment_ids(sizes)
    X = gr.randn32((len(bb), D), 31)
    sc, sh = gr.pro_scale_shift(D, 32) if pro else (None, None)
    sums = gr.emulate_run_sum(X.numpy(), ptr, trip=8, scale=None if not pro else sc.numpy(),
                              shift=None if not pro else sh.numpy(), relu=pro, defect=defect)
    got = gr.emulate_mean(sums, ptr, divides=True, defect=mean_defect)
    want, tol, cnt = gr.csr_mean_fwd_ref(X, sc, sh, pro, torch.from_numpy(bb), len(sizes), divides=True)
    return got, want, tol, cnt


@pytest.mark.parametrize("pro", [False, True])
def test_segment_mean_envelope_accepts_the_emulation_and_rejects_every_defect(pro):
    got, want, tol, cnt = _segment_mean(pro)
    ok, worst = _inside(got, want, tol)
    assert ok, worst
    assert (got[(cnt == 0).numpy()] == 0).all()
    for defect in gr.RUN_DEFECTS:
        got, want, tol, _ = _segment_mean(pro, defect=defect)
        ok, worst = _inside(got, want, tol)
        assert not ok and worst > 100.0, (defect, worst)
    got, want, tol, cnt = _segment_mean(pro, mean_defect="deg_divisor")
    bad = ~((torch.from_numpy(got).double() - want).abs() <= tol)
    assert bool(bad[cnt == 0].all()) and not bool(bad[cnt > 0].any())
    # the backward: one division
    dY = gr.randn32((len(cnt), 20), 33)
    q = dY.double() / cnt.clamp_min(1)[:, None]
    got = dY / cnt.clamp_min(1).float()[:, None]
    ok, worst = _inside(got, q, gr.segment_mean_bwd_tol(q))
    assert ok and worst > 0.0


def test_first_argmax_takes_the_lowest_row_of_a_tie_and_marks_an_empty_run():
    x = np.array([[1.0, 5.0], [3.0, 5.0], [3.0, -1.0], [-2.0, -2.0], [-2.0, -3.0]], dtype=F32)
    best, arg = gr.first_argmax(x, np.array([0, 3, 3, 5]), 5)
    assert best.tolist() == [[3.0, 5.0], [0.0, 0.0], [-2.0, -2.0]]
    assert arg.tolist() == [[1, 0], [5, 5], [3, 3]]


@pytest.mark.parametrize("with_b1", [False, True])
@pytest.mark.parametrize("E,kind", gr.EDGE_CASES)
def test_uv_lin1_envelope_accepts_the_emulation(E, kind, with_b1):
    N, src, dst = gr.edge_case_graph(E, kind)
    order = np.argsort(dst, kind="stable")
    s, d = torch.from_numpy(src[order]), torch.from_numpy(dst[order])
    UV = gr.randn32((N, 128), 3 * E + N)
    attr = gr.randn32((E, 4), 3 * E + N + 3, 0.5)
    wc4 = gr.randn32((64, 4), 3 * E + N + 1, 0.5)
    b1 = gr.randn32((64,), 3 * E + N + 2, 0.3) if with_b1 else None

    def emulate(v_rows):                                   # k_edge_uv_lin1's `one`: u + v, four fmas, + b
        z = (UV[:, :64][d] + UV[:, 64:][v_rows]).numpy()
        for j in range(4):
            z = gr.fma32(attr.numpy()[:, j:j + 1], wc4.numpy()[None, :, j], z)
        return z + b1.numpy() if with_b1 else z
    want, delta = gr.edge_uv_lin1_ref(UV, s, d, attr, wc4, b1)
    ok, worst = _inside(emulate(s), want, delta)
    assert ok, worst
    if bool((s != d).any()):                               # the V half read at the destination instead of the source
        assert not _inside(emulate(d), want, delta)[0]
    # the BatchNorm partials of the kernel's epilogue, per 32-row group (the last one short), inside group_stats_ref's bounds
    gs, gm2 = gr.emulate_group_stats(emulate(s))
    ws, wm2, ts, tm = gr.group_stats_ref(want, delta)
    assert gs.shape == ws.shape == (-(-E // 32), 64)
    for got, w, t in ((gs, ws, ts), (gm2, wm2, tm)):
        ok, worst = _inside(got, w, t)
        assert ok, worst
    if E % 32 != 1:                                        # a last group divided by 32 instead of its row count is outside
        cnt = E - 32 * (E // 32) or 32
        h = emulate(s)[32 * ((E - 1) // 32):]
        mu_bad = h.sum(0) / F32(32) if cnt != 32 else h.sum(0) / F32(31)
        m2_bad = ((h - mu_bad) ** 2).sum(0)
        assert not _inside(m2_bad, wm2[-1], tm[-1])[0]


# ---------------------------------------------------------------------------------------------
# BnCsrGrad: the envelopes accept the emulation at every case; the cross-tile defect shows only at the multi-tile cases
# ---------------------------------------------------------------------------------------------
_BN_CACHE = {}


def _bn_case(N, E, kind):
    key = (N, E, kind)
    if key not in _BN_CACHE:
        src, dst = gr.bn_csr_graph(N, E, kind)
        d = torch.from_numpy(np.sort(dst, kind="stable"))
        inp = gr.bn_csr_inputs(N, E, 5 * N + E)
        _BN_CACHE.clear()                                  # one case at a time: the multi-tile ones are [65537, 64]
        _BN_CACHE[key] = (d, inp)
    return _BN_CACHE[key]


def _bn_judge(N, E, kind, defect=None):
    """{output name: (inside, worst ratio)} of the emulation against every envelope of the GPU test"""
    d, inp = _bn_case(N, E, kind)
    emu = gr.emulate_bn_csr(inp, d, N, defect=defect)
    ref, g0, tol_b, tol_g = gr.bn_csr_stats_ref(inp["d_out"], d, N, inp["Y"], inp["mean"], inp["invstd"], inp["scale"],
                                                inp["shift"])
    res = {"dbeta": _inside(emu["dbeta"], ref["dbeta"], tol_b), "dgamma": _inside(emu["dgamma"], ref["dgamma"], tol_g),
           "c1": _inside(emu["coef"][:64], ref["c1"], tol_b / E), "c2": _inside(emu["coef"][64:], ref["c2"], tol_g / E)}
    dY, d_dY = gr.bn_csr_dy_ref(g0, inp["Y"], inp["mean"], inp["invstd"], inp["scale"], inp["shift"], emu["coef"])
    con = gr.bn_csr_consumers_ref(dY, d_dY, inp["A"], inp["a_scale"], inp["a_shift"], True, inp["W"])
    for k in ("dW", "db", "dA"):
        res[k] = _inside(emu[k], con[k], con["tol_" + k])
    nb, t1, ng, t2 = gr.next_bn_ref(emu["dA"], inp["A"], inp["a_scale"], inp["a_shift"], inp["m1"], inp["is1"])
    res["next dbeta"] = _inside(emu["next_dbeta"], nb, t1)
    res["next dgamma"] = _inside(emu["next_dgamma"], ng, t2)
    res["next c1"] = _inside(emu["next_coef"][:64], nb / E, t1 / E)
    res["next c2"] = _inside(emu["next_coef"][64:], ng / E, t2 / E)
    return res


@pytest.mark.parametrize("N,E,kind", gr.BN_CSR_CASES)
def test_bn_csr_envelopes_accept_the_emulation(N, E, kind):
    res = _bn_judge(N, E, kind)
    assert all(ok for ok, _ in res.values()), res
    tiles, per, wgs = gr.l2_tiles(E)
    assert (tiles, per, wgs) == {31: (1, 1, 1), 64: (1, 1, 1), 65: (2, 1, 2), 129: (3, 1, 3), 1000: (16, 1, 16),
                                 32769: (513, 2, 257), 65537: (1025, 3, 342)}[E]
    assert (tiles - 1) % per + 1 == {32769: 1, 65537: 2}.get(E, 1)   # tiles of the last workgroup


@pytest.mark.parametrize("N,E,kind", gr.BN_CSR_MULTI_TILE)
def test_bn_csr_envelopes_reject_sums_lost_between_the_tiles_of_a_workgroup(N, E, kind):
    res = _bn_judge(N, E, kind, defect="tile_loss")
    for k in ("dW", "db", "next dbeta", "next dgamma", "next c1", "next c2"):
        assert not res[k][0] and res[k][1] > 5.0, (k, res[k])      # far outside, not a borderline element
    for k in ("dbeta", "dgamma", "c1", "c2", "dA"):                  # not carried from tile to tile: untouched
        assert res[k][0], (k, res[k])


def test_the_cross_tile_defect_is_invisible_below_32769_edges():
    """why the two multi-tile cases are there: with one tile per workgroup (every op-level case so far) a kernel that
    loses its accumulators between tiles computes the same bits"""
    d, inp = _bn_case(300, 1000, "hub150")
    a, b = gr.emulate_bn_csr(inp, d, 300), gr.emulate_bn_csr(inp, d, 300, defect="tile_loss")
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("N,E,kind", [(300, 1000, "hub150"), (64, 65, "uniform")])
def test_bn_csr_envelopes_reject_a_duplicated_row_and_a_missing_degree(N, E, kind):
    res = _bn_judge(N, E, kind, defect="row_dup")
    assert not res["dA"][0] and not res["db"][0] and not res["dW"][0], res
    res = _bn_judge(N, E, kind, defect="no_inv_deg")
    assert not res["dbeta"][0] and not res["dgamma"][0], res
