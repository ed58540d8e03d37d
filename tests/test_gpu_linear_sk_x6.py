"""yolat_linear_sk_x6 (csrc/linear_sk_x6.hip): the LDS-DMA split-K Linear with its products on the bf16 matrix cores
(bf16x6-emulated fp32), and its place in the eval forward (classifier 1 at few proposals, YOLAT_CLS1_SK_X6).

Operator level, against an fp64 product on the CPU with the whole epilogue (bias, scale, shift, ReLU on and off):
  K in {128 (one chunk, no prefetch), 256 (each LDS stage once), 384 (a stage re-used, odd chunk count), 1152},
  M in {1, 31, 33, 65} (row clamping, partial row tiles, three row tiles), N in {1, 17, 33} (column clamping),
  lda = K and K + 8, ldb = K + 4, inputs with negatives and exact zeros.
The bound is not fixed in advance: the fp32-input MFMA kernel behind yolat_linear_fwd runs on the same inputs, its
largest error normalised by sum_k |a_k| |w_k| * |scale| over the cases of one K is the yardstick, and the new kernel is
allowed 4 x that (another summation grouping plus the three dropped O(2^-24) cross terms per product: the same precision
class).  Both figures are printed before the assertion.

Forward level, in child processes (the switches are read once per process)."""
import os
import subprocess
import sys

import pytest
import torch

from yolat_vectorgraphicsrecognition_amd import _lib, ops

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS, NS = (1, 31, 33, 65), (1, 17, 33)
UNSUPPORTED = -2


def _inputs(M, N, K, lda, ldb, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, lda, generator=g)
    W = torch.randn(N, ldb, generator=g) * 0.05
    A[torch.rand(M, lda, generator=g) < 0.1] = 0.0          # exact zeros
    W[torch.rand(N, ldb, generator=g) < 0.1] = 0.0
    bias = torch.randn(N, generator=g)
    scale = torch.randn(N, generator=g)                      # both signs
    scale[scale.abs() < 0.05] = 0.5
    shift = torch.randn(N, generator=g)
    return A, W, bias, scale, shift


def _reference(A, W, bias, scale, shift, K, relu):
    a, w = A[:, :K].double(), W[:, :K].double()
    y = (a @ w.t() + bias.double()) * scale.double() + shift.double()
    norm = (a.abs() @ w.abs().t()) * scale.double().abs()
    return (y.clamp_min(0.0) if relu else y), norm


@pytest.mark.parametrize("K", [128, 256, 384, 1152])
def test_linear_sk_x6_against_fp64_within_4x_of_the_fp32_mfma_kernel(K):
    worst_new, worst_old, seed = 0.0, 0.0, 0
    for M in MS:
        for N in NS:
            for lda in (K, K + 8):
                seed += 1
                A, W, bias, scale, shift = _inputs(M, N, K, lda, K + 4, 1000 * K + seed)
                dev = [t.cuda() for t in (A, W, bias, scale, shift)]
                a_d, w_d = dev[0][:, :K], dev[1][:, :K]              # row views: lda / ldb are the strides
                for relu in (False, True):
                    want, norm = _reference(A, W, bias, scale, shift, K, relu)
                    assert float(norm.min()) > 0.0
                    y_new = torch.full((M, N), float("nan"), device="cuda")
                    y_new2 = torch.full((M, N), float("nan"), device="cuda")
                    y_old = torch.full((M, N), float("nan"), device="cuda")
                    ops.linear_sk_x6(a_d, w_d, dev[2], y_new, o_pro=(dev[3], dev[4]), o_relu=relu)
                    ops.linear_sk_x6(a_d, w_d, dev[2], y_new2, o_pro=(dev[3], dev[4]), o_relu=relu)
                    ops.linear_fwd(a_d, w_d, dev[2], y_old, o_pro=(dev[3], dev[4]), o_relu=relu)
                    assert torch.isfinite(y_new).all() and torch.isfinite(y_old).all()
                    assert torch.equal(y_new, y_new2), (M, N, lda, relu)            # two calls: bit-equal
                    worst_new = max(worst_new, float(((y_new.cpu().double() - want).abs() / norm).max()))
                    worst_old = max(worst_old, float(((y_old.cpu().double() - want).abs() / norm).max()))
    print("K=%d: largest normalised error: fp32 MFMA kernel %.3e, LDS-DMA bf16x6 kernel %.3e" % (K, worst_old, worst_new))
    assert worst_old > 0.0
    assert worst_new <= 4.0 * worst_old


def test_linear_sk_x6_declines_shapes_outside_its_contract():
    A = torch.randn(8, 400, device="cuda")
    W = torch.randn(16, 400, device="cuda")
    Y = torch.zeros(8, 16, device="cuda")

    def call(a, lda, K, w, ldw):
        return _lib.lib.yolat_linear_sk_x6(a, lda, 8, K, w, ldw, None, 16, None, None, 0, Y.data_ptr(), 16, None)
    assert call(A.data_ptr(), 400, 100, W.data_ptr(), 400) == UNSUPPORTED              # K % 128 != 0
    assert call(A.data_ptr(), 400, 64, W.data_ptr(), 400) == UNSUPPORTED               # K < 128
    assert call(A.data_ptr(), 398, 256, W.data_ptr(), 400) == UNSUPPORTED              # rows of A not 16-byte aligned
    assert call(A.data_ptr(), 400, 256, W.data_ptr(), 398) == UNSUPPORTED              # rows of W not 16-byte aligned
    assert call(A.data_ptr() + 4, 396, 256, W.data_ptr(), 400) == UNSUPPORTED          # A itself misaligned
    assert call(A.data_ptr(), 400, 256, W.data_ptr() + 8, 396) == UNSUPPORTED          # W itself misaligned
    torch.cuda.synchronize()
    assert float(Y.abs().max()) == 0.0                                                 # nothing was launched
    assert call(A.data_ptr(), 400, 256, W.data_ptr(), 400) == 0
    torch.cuda.synchronize()
    assert float(Y.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------
# the eval forward: default vs YOLAT_CLS1_SK_X6=0, with and without YOLAT_STRICT_FP32=1
# ---------------------------------------------------------------------------------------------
_SCRIPT = (
    "import sys, torch\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import golden_util as gu\n"
    "import yolat_vectorgraphicsrecognition_amd as yv\n"
    "data, slices = yv.synth_batch(2, 7, num_proposals=37, nodes_lo=2, nodes_hi=30)\n"
    "model = gu.fill_state_(yv.SparseCADGCN(yv.Opt()), 3).cuda().eval()\n"
    "with torch.no_grad():\n"
    "    logits = model(data, slices)[0].cpu()\n"
    "model.check_last_status()\n"
    "torch.save(logits, sys.argv[1])\n" % (REPO, os.path.join(REPO, "tests")))
_RUNS = (("default", {}), ("off", {"YOLAT_CLS1_SK_X6": "0"}), ("strict", {"YOLAT_STRICT_FP32": "1"}),
         ("strict_off", {"YOLAT_STRICT_FP32": "1", "YOLAT_CLS1_SK_X6": "0"}))


@pytest.fixture(scope="module")
def forward_logits(tmp_path_factory):
    """logits of the same small forward under the four switch settings: four child processes side by side"""
    tmp = tmp_path_factory.mktemp("cls1_sk_x6")
    base = {k: v for k, v in os.environ.items() if k not in ("YOLAT_CLS1_SK_X6", "YOLAT_STRICT_FP32")}
    procs = []
    for tag, env in _RUNS:
        out = str(tmp / ("logits_%s.pt" % tag))
        procs.append((tag, out, subprocess.Popen([sys.executable, "-c", _SCRIPT, out], env=dict(base, **env))))
    got = {}
    for tag, out, p in procs:
        assert p.wait(timeout=600) == 0, tag
        got[tag] = torch.load(out)
    return got


def test_forward_takes_the_new_kernel_and_stays_within_the_x6_bar(forward_logits):
    a, b = forward_logits["default"], forward_logits["off"]
    assert a.shape == b.shape and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert not torch.equal(a, b)                                   # classifier 1 ran on another kernel
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print("default vs YOLAT_CLS1_SK_X6=0: max |diff| %.3e of scale %.3e" % (err, scale))
    assert err <= 1e-5 * scale


def test_strict_fp32_keeps_the_fp32_mfma_kernel(forward_logits):
    a, b = forward_logits["strict"], forward_logits["strict_off"]
    assert torch.isfinite(a).all() and torch.equal(a, b)
