"""The reference helpers of tests/bf16_ref.py are what they claim to be (no GPU needed): the rounding helpers, the
envelope (it accepts an fp32 emulation of the bf16-storage Linear and rejects two wrong stores), the exact-prologue grid,
the ReLU-kink condition on the BatchNorm inputs and the graph builders."""
import numpy as np
import pytest
import torch

import bf16_ref as br

pytestmark = pytest.mark.host

LIN_SHAPES = [(1, 64, 64), (33, 64, 64), (65, 64, 64), (4099, 64, 64), (300, 128, 34)]


def _linear_case(M, K, Nout, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + M + K + Nout)
    A = br.grid_activation(M, K, seed + M)
    scale, shift = br.grid_scale_shift(K, seed + K)
    W = torch.randn(Nout, K, generator=g) / 8
    bias = torch.randn(Nout, generator=g) * 0.1
    return A, scale, shift, W, bias


def test_bf_rounds_to_nearest_even_and_agrees_with_torch_on_fp32():
    x = torch.randn(20001, generator=torch.Generator().manual_seed(0)) * 3.0
    assert torch.equal(br.bf(x), br.bf(x.double()))                   # fp32 values: one rounding either way
    # ties: 1 + 2^-8 is halfway between 1 and 1 + 2^-7 -> even (1); 1 + 3 2^-8 -> 1 + 2^-6
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0], dtype=torch.float64)
    assert br.bf(t).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 0.0]
    # float64 input is rounded ONCE: 1 + 2^-8 + 2^-40 lies above the tie (through fp32 it would collapse onto it)
    assert float(br.bf(torch.tensor(1.0 + 2.0 ** -8 + 2.0 ** -40, dtype=torch.float64))) == 1.0 + 2.0 ** -7
    assert br.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -3.0, 0.75])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6,
                                                                              2.0 ** -8]
    assert float(br.ulp_bf16(0.0)) == 2.0 ** -133
    y = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -9, -1.0 - 2.0 ** -7 - 2.0 ** -9])
    assert br.truncate_bf16(y).double().tolist() == [1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7]       # towards zero


def test_store_envelope_is_half_a_spacing_plus_delta():
    want = torch.tensor([1.0, 1.9999, 0.0, -5.0], dtype=torch.float64)
    tol = br.store_envelope(want, torch.tensor([0.0, 0.001, 0.0, 0.25], dtype=torch.float64))
    # 1.9999 + 0.001 crosses 2: the spacing of the next binade; -5 -> spacing 2^-5
    assert tol.tolist() == [2.0 ** -8, 2.0 ** -7 + 0.001, 2.0 ** -134, 2.0 ** -6 + 0.25]


@pytest.mark.parametrize("M,K,Nout", LIN_SHAPES)
def test_grid_prologue_is_exact_in_fp32(M, K, Nout):
    A, scale, shift, _, _ = _linear_case(M, K, Nout)
    assert A.dtype == torch.bfloat16 and float(A.double().abs().max()) <= 4.0
    assert torch.equal(A.double() * 64, (A.double() * 64).round())
    assert set((scale * 8).tolist()) <= set(range(4, 13)) and float((shift * 64).abs().max()) <= 64
    assert br.prologue_is_exact_in_fp32(A, scale, shift)
    # ... hence re-rounding to bfloat16 is the same function in fp32 and in float64
    for relu in (False, True):
        z32 = A.float() * scale + shift
        z32 = torch.relu(z32) if relu else z32
        assert torch.equal(z32.to(torch.bfloat16).double(), br.bf(br.prologue(A, scale, shift, relu)))


@pytest.mark.parametrize("M,K,Nout", LIN_SHAPES)
@pytest.mark.parametrize("pro", ["none", "affine", "relu"])
def test_store_envelope_accepts_the_fp32_round_to_nearest_emulation(M, K, Nout, pro):
    A, scale, shift, W, bias = _linear_case(M, K, Nout)
    sc, sh = (None, None) if pro == "none" else (scale, shift)
    got = br.emulate_linear_fwd_h(A, sc, sh, pro == "relu", W, bias).double()
    want, delta = br.linear_fwd_ref(A, sc, sh, pro == "relu", W, bias)
    tol = br.store_envelope(want, delta)
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())


@pytest.mark.parametrize("M,K,Nout", LIN_SHAPES)
def test_store_envelope_rejects_a_truncating_store(M, K, Nout):
    A, scale, shift, W, bias = _linear_case(M, K, Nout)
    got = br.emulate_linear_fwd_h(A, scale, shift, True, W, bias, store="truncate").double()
    want, delta = br.linear_fwd_ref(A, scale, shift, True, W, bias)
    bad = (got - want).abs() > br.store_envelope(want, delta)
    assert float(bad.double().mean()) > 0.25, float(bad.double().mean())


@pytest.mark.parametrize("M,K,Nout", [s for s in LIN_SHAPES if s[0] >= 2])
def test_store_envelope_rejects_a_duplicated_last_row(M, K, Nout):
    A, scale, shift, W, bias = _linear_case(M, K, Nout)
    got = br.emulate_linear_fwd_h(A, scale, shift, True, W, bias, dup_last_row=True).double()
    want, delta = br.linear_fwd_ref(A, scale, shift, True, W, bias)
    bad = (got - want).abs() > br.store_envelope(want, delta)
    assert not bool(bad[:-1].any())
    assert float(bad[-1].double().mean()) > 0.5                     # the wrong row is off in most of its columns


def test_group_stats_ref_matches_a_direct_computation_and_bounds_an_fp32_one():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(70, 5, generator=g).double() * 2 + 1
    s, m2, ts, tm = br.group_stats_ref(v, torch.zeros_like(v))
    assert s.shape == (3, 5)
    for gi, (lo, hi) in enumerate([(0, 32), (32, 64), (64, 70)]):
        blk = v[lo:hi]
        assert torch.allclose(s[gi], blk.sum(0), rtol=1e-14, atol=0)
        assert torch.allclose(m2[gi], ((blk - blk.mean(0)) ** 2).sum(0), rtol=1e-13, atol=0)
        # the same in fp32 stays inside the tolerances
        b32 = blk.float()
        assert bool(((b32.sum(0).double() - s[gi]).abs() <= ts[gi] + 32 * br.EPS32 * blk.abs().sum(0)).all())
    assert bool((ts > 0).all() and (tm > 0).all())


@pytest.mark.parametrize("M", [1, 63, 65, 1000, 262144 + 70])
@pytest.mark.parametrize("C", [64, 128])
def test_bn_bwd_inputs_stay_off_the_relu_kink(M, C):
    Y, dZ, mean, invstd, scale, shift = br.bn_bwd_inputs(M, C, seed=M + C)
    assert Y.dtype == dZ.dtype == torch.bfloat16 and Y.shape == dZ.shape == (M, C)
    assert all(t.dtype == torch.float32 and t.shape == (C,) for t in (mean, invstd, scale, shift))
    assert br.kink_share(Y, scale, shift) <= br.KINK_SHARE
    if M <= 1000:
        y = Y.double()
        assert torch.allclose(mean.double(), y.mean(0), rtol=1e-6, atol=1e-7)
        assert torch.allclose(invstd.double(), 1 / torch.sqrt(y.var(0, unbiased=False) + 1e-5), rtol=1e-6)


def test_bn_relu_bwd_ref_is_the_autograd_of_batchnorm_relu_and_of_the_mean_aggregation():
    M, C, N = 300, 8, 40
    Y, dZ, mean, invstd, scale, shift = br.bn_bwd_inputs(M, C, seed=5)
    y = Y.double().requires_grad_(True)
    gamma = (scale.double() / invstd.double()).requires_grad_(True)
    beta = (shift.double() + mean.double() * scale.double()).requires_grad_(True)
    z = torch.relu(torch.nn.functional.batch_norm(y, None, None, gamma, beta, True, 0.0, 1e-5))
    z.backward(dZ.double())
    ref = br.bn_relu_bwd_ref(dZ, Y, mean, invstd, scale, shift, True)
    # (the statistics handed to the restatement are the fp32-rounded ones: 1e-6)
    assert torch.allclose(ref["dY"], y.grad, rtol=0, atol=2e-6 * float(y.grad.abs().max()))
    assert torch.allclose(ref["dgamma"], gamma.grad, rtol=0, atol=2e-6 * float(gamma.grad.abs().max()))
    assert torch.allclose(ref["dbeta"], beta.grad, rtol=0, atol=2e-6 * float(beta.grad.abs().max()))
    # mean aggregation in front: d_out [N,C] -> per-edge gradient
    src, dst = br.hub(N + 110, M, 65, seed=1)
    dst = torch.from_numpy(dst)
    d_out = torch.randn(N + 110, C, generator=torch.Generator().manual_seed(2)).double()
    m = torch.randn(M, C, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    out, mag, deg = br.csr_mean_ref(m, dst, N + 110)
    out.backward(d_out)
    assert torch.allclose(br.csr_mean_bwd_ref(d_out, dst, N + 110), m.grad, rtol=1e-14, atol=0)
    assert torch.equal(deg.long(), torch.from_numpy(br.in_degree(dst.numpy(), N + 110)))


@pytest.mark.parametrize("deg", [65, 150, 1000])
def test_hub_graph_has_the_stated_degrees_and_empty_run(deg):
    N, E = 300, 2000
    src, dst = br.hub(N, E, deg, seed=deg)
    assert src.dtype == dst.dtype == np.int64 and src.shape == dst.shape == (E,)
    assert src.min() >= 0 and dst.min() >= 0 and src.max() < N and dst.max() < N
    din, dout = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    assert din[br.HUB_IN] == deg and dout[br.HUB_OUT] == deg
    assert -(-deg // 64) == {65: 2, 150: 3, 1000: 16}[deg]           # 64-row tiles a segment of deg rows spans at least
    quiet = np.arange(N - 1 - br.QUIET, N - 1)
    assert len(quiet) >= 130 and not din[quiet].any() and dout[quiet].any()
    assert din[N - 1] == 0 and dout[N - 1] == 0
    assert (din[:N - 1 - br.QUIET] > 0).sum() > 100                   # the rest is an ordinary random graph
    with pytest.raises(ValueError):
        br.hub(300, 2 * deg - 1, deg)


def test_chain_and_uniform_graphs():
    src, dst = br.chain(257)
    assert src.dtype == dst.dtype == np.int64 and len(src) == 257
    assert (np.bincount(dst, minlength=257) == 1).all() and (np.bincount(src, minlength=257) == 1).all()
    assert (src != dst).all()
    src, dst = br.uniform(40000, 9000, seed=1)
    assert src.dtype == dst.dtype == np.int64 and len(src) == 9000 and src.max() < 40000 and dst.max() < 40000
    assert (np.bincount(dst, minlength=40000) == 0).sum() > 30000     # most nodes have no in-edge
    a, b = br.uniform(40000, 9000, seed=1)
    assert np.array_equal(a, src) and np.array_equal(b, dst)          # seeded
