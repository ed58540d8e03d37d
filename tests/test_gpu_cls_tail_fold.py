"""GPU tests (-m gpu) of classifier layers 2 + 3 of the fp32 eval forward as one launch (csrc/cls_tail.hip k_cls_tail:
layer 2 on k_gemm_nt_sk's 32 x 32 tiles, layer 3 as per-tile partial products that the last workgroup of a row tile sums).

Through yolat_debug_cls_tail_eval, the pair routed as the forward routes it:
  * P in {1, 31, 32, 33, 95, 400} x H1 in {128, 384, 512} (one, three, four 128-deep chunks: H1 = 128 is below the split-K
    kernel's K >= 256 and takes the two launches; 384 and 512 leave the two-register-set loop by its two exits) x H2 in
    {32, 96, 256} (one, three, eight column tiles: with one tile the first arriver is the reducer) x n_classes in {1, 17, 32}:
    c2 must hold the BYTES of yolat_linear_fwd's c2; every logit must lie within
        (H2 + 8) 2^-24 sum_k |c2_k W3_ck|  +  2^-23 |value|
    of the float64 product of that c2 with W3 (+ b3): the fp32 dot-product bound of any summation order over H2 products
    (gamma_n <= (n + 8) u for the H2 products and H2 - 1 additions at n <= 2^10); the bias addition and the final rounding
    are the 2^-23 |value| term.  Nothing measured enters it.
  * n_classes = 33 and H2 = 48 are outside the fold: the op reports the two launches and returns their bytes.
  * one work buffer, never cleared in between: three calls back to back, a smaller P, a larger P, the first shape again —
    every call equals the first result of its shape byte for byte (tickets left at zero by every launch; an un-primed call
    zeroes them itself, on a buffer filled with ones).
  * 200 calls at P = 400 while a second stream copies 256 MB buffers back and forth (uneven load): every word equals the
    idle result.

Model level: the eval forward of a small model with YOLAT_CLS_TAIL_FOLD unset and = 0 (read once: two child processes),
each under both launch regimes.  Boxes byte-equal; the logits of the two settings are two fp32 summations of the same c2, so
they differ by at most twice the bound above — c2 and W3 taken from the float64 oracle model, whose c2 differs from the
device's by the upstream layers' ~1e-5 relative error: the bound is widened by 1e-3 of itself for that."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PS, H1S, H2S, NCS = (1, 31, 32, 33, 95, 400), (128, 384, 512), (32, 96, 256), (1, 17, 32)


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _fns():
    lib = _yv()._lib.lib
    p, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.yolat_debug_cls_tail_eval
    fn.restype = ci
    fn.argtypes = [p, i64, i64, i64, p, i64, p, p, p, i64, p, i64, p, i64, p, i64, p, ci, p, i64, ctypes.POINTER(ci), p]
    wb = lib.yolat_debug_cls_tail_work_bytes
    wb.restype = ctypes.c_size_t
    wb.argtypes = [i64, i64]
    return fn, wb


_POOL = {}


def _pool():
    """one set of operands at the largest sizes; every case takes its leading rows / columns"""
    if not _POOL:
        g = torch.Generator().manual_seed(20)
        rn = lambda *s: torch.randn(*s, generator=g)
        _POOL.update(c1=rn(400, 512).clamp_(min=0), W2=rn(256, 512) / 16, b2=rn(256) * 0.1, s2=torch.rand(256, generator=g) + 0.5,
                     t2=rn(256) * 0.2, W3=rn(33, 256) / 8, b3=rn(33) * 0.1)
    return _POOL


def _operands(P, H1, H2, nc):
    z = _pool()
    cut = dict(c1=z["c1"][:P, :H1], W2=z["W2"][:H2, :H1], b2=z["b2"][:H2], s2=z["s2"][:H2], t2=z["t2"][:H2], W3=z["W3"][:nc, :H2],
               b3=z["b3"][:nc])
    return {k: v.contiguous().cuda() for k, v in cut.items()}


def _run(d, P, H1, H2, nc, work, primed, logits=None):
    """(logits, c2, folded) of one call of the op on `work`"""
    fn, wb = _fns()
    assert work.numel() * 4 >= wb(P, H2) and work.data_ptr() % 256 == 0
    if logits is None:
        logits = torch.full((P, nc), float("nan"), device="cuda")
    c2 = torch.full((P, H2), float("nan"), device="cuda")
    folded = ctypes.c_int(-1)
    rc = fn(d["c1"].data_ptr(), H1, P, H1, d["W2"].data_ptr(), H1, d["b2"].data_ptr(), d["s2"].data_ptr(), d["t2"].data_ptr(), H2,
            d["W3"].data_ptr(), H2, d["b3"].data_ptr(), nc, logits.data_ptr(), logits.stride(0), work.data_ptr(), int(primed),
            c2.data_ptr(), H2, ctypes.byref(folded), _yv().ops._stream())
    assert rc == 0, (rc, P, H1, H2, nc)
    return logits, c2, folded.value


def _work(P, H2):
    _, wb = _fns()
    return torch.ones(wb(P, H2) // 4, dtype=torch.int32, device="cuda")        # never zero: the op's un-primed call zeroes


def _two_launches(d, P, H2, nc):
    yv = _yv()
    c2 = yv.ops.linear_fwd(d["c1"], d["W2"], d["b2"], torch.empty(P, H2, device="cuda"), o_pro=(d["s2"], d["t2"]), o_relu=True)
    return c2, yv.ops.linear_fwd(c2, d["W3"], d["b3"], torch.empty(P, nc, device="cuda"))


@pytest.mark.parametrize("H1", H1S)
@pytest.mark.parametrize("P", PS)
def test_c2_bytes_and_logits_within_the_dot_product_bound(P, H1):
    worst = 0.0
    for H2 in H2S:
        for nc in NCS:
            d = _operands(P, H1, H2, nc)
            logits, c2, folded = _run(d, P, H1, H2, nc, _work(P, H2), primed=False)
            assert folded == (1 if H1 >= 256 else 0), (P, H1, H2, nc, folded)
            want_c2, _ = _two_launches(d, P, H2, nc)
            assert torch.equal(c2.view(torch.int32), want_c2.view(torch.int32)), ("c2 bytes", P, H1, H2, nc)
            c2d, w3d = want_c2.double().cpu(), d["W3"].double().cpu()
            ref = c2d @ w3d.t() + d["b3"].double().cpu()
            mag = c2d.abs() @ w3d.abs().t()
            bound = (H2 + 8) * U * mag + 2 * U * ref.abs()
            err = (logits.double().cpu() - ref).abs()
            assert torch.isfinite(logits).all(), (P, H1, H2, nc)
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
            assert bool((err <= bound).all()), ("logits", P, H1, H2, nc, float((err / bound.clamp(min=1e-300)).max()))
    print("P = %d, H1 = %d: worst error / bound %.3f" % (P, H1, worst))


@pytest.mark.parametrize("H2,nc", [(256, 33), (48, 17)])
def test_shapes_outside_the_fold_return_the_two_launch_result(H2, nc):
    z = _pool()
    g = torch.Generator().manual_seed(3)
    d = dict(c1=z["c1"][:95, :384], W2=z["W2"][:H2, :384], b2=z["b2"][:H2], s2=z["s2"][:H2], t2=z["t2"][:H2],
             W3=torch.randn(nc, H2, generator=g) / 8, b3=z["b3"][:nc])
    d = {k: v.contiguous().cuda() for k, v in d.items()}
    logits, c2, folded = _run(d, 95, 384, H2, nc, _work(95, H2), primed=False)
    want_c2, want = _two_launches(d, 95, H2, nc)
    assert folded == 0
    assert torch.equal(c2.view(torch.int32), want_c2.view(torch.int32)) and torch.equal(logits.view(torch.int32), want.view(torch.int32))


def test_one_work_buffer_across_calls_and_shapes():
    H1, H2, nc = 512, 256, 17
    work = _work(400, H2)
    first = {}
    for P, primed in ((95, False), (95, True), (95, True), (33, False), (400, False), (400, True), (95, False), (95, True)):
        d = _operands(P, H1, H2, nc)
        logits, _, folded = _run(d, P, H1, H2, nc, work, primed)
        assert folded == 1 and torch.isfinite(logits).all()
        if P not in first:
            first[P] = logits.clone()
        assert torch.equal(logits.view(torch.int32), first[P].view(torch.int32)), (P, primed)
    torch.cuda.synchronize()


def test_200_calls_under_uneven_load_equal_the_idle_result():
    P, H1, H2, nc = 400, 512, 256, 17
    d = _operands(P, H1, H2, nc)
    work = _work(P, H2)
    idle, _, folded = _run(d, P, H1, H2, nc, work, primed=False)
    assert folded == 1
    torch.cuda.synchronize()
    a = torch.empty(64 << 20, dtype=torch.float32, device="cuda")           # 256 MB
    b = torch.empty_like(a)
    out = torch.full((200, P, nc), float("nan"), device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(12):
            b.copy_(a, non_blocking=True)
            a.copy_(b, non_blocking=True)
    for i in range(200):
        _run(d, P, H1, H2, nc, work, True, logits=out[i])
    busy = not side.query()
    torch.cuda.synchronize()
    print("side stream still copying when the last call was enqueued:", busy)
    same = (out.view(torch.int32) == idle.view(torch.int32).unsqueeze(0)).all(dim=2).all(dim=1)
    assert bool(same.all()), "calls that differ from the idle result: %s" % (~same).nonzero().flatten().tolist()[:20]


# ---------------------------------------------------------------------------------------------
# the eval forward: YOLAT_CLS_TAIL_FOLD unset vs = 0, under both launch regimes
# ---------------------------------------------------------------------------------------------
_SCRIPT = (
    "import sys, torch\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import golden_util as gu\n"
    "import yolat_vectorgraphicsrecognition_amd as yv\n"
    "lib = yv._lib.lib\n"
    "data, slices = yv.synth_batch(2, 7, num_proposals=37, nodes_lo=2, nodes_hi=30)\n"
    "model = gu.fill_state_(yv.SparseCADGCN(yv.Opt()), 3).cuda().eval()\n"
    "out = {}\n"
    "for name, mode in (('latency', 1), ('throughput', 2)):\n"
    "    assert lib.yolat_eval_regime_set(mode) == 0\n"
    "    with torch.no_grad():\n"
    "        for rep in range(3):\n"                                    # the third forward of a shape runs primed
    "            got = model(data, slices)\n"
    "            out['%%s_%%d' %% (name, rep)] = (got[0].cpu(), got[1].cpu())\n"
    "    model.check_last_status()\n"
    "torch.save(out, sys.argv[1])\n" % (REPO, os.path.join(REPO, "tests")))


@pytest.fixture(scope="module")
def forwards(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cls_tail_fold")
    base = {k: v for k, v in os.environ.items() if k not in ("YOLAT_CLS_TAIL_FOLD", "YOLAT_STRICT_FP32", "YOLAT_EVAL_REGIME")}
    procs = []
    for tag, env in (("on", {}), ("off", {"YOLAT_CLS_TAIL_FOLD": "0"})):
        out = str(tmp / ("forward_%s.pt" % tag))
        procs.append((tag, out, subprocess.Popen([sys.executable, "-c", _SCRIPT, out], env=dict(base, **env))))
    got = {}
    for tag, out, p in procs:
        assert p.wait(timeout=600) == 0, tag
        got[tag] = torch.load(out)
    return got


def _oracle_c2_w3():
    """c2 and the last layer of the float64 oracle model on the forwards' batch"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import golden_util as gu
    from oracle import oracle_torch as orc
    yv = _yv()
    data, slices = yv.synth_batch(2, 7, num_proposals=37, nodes_lo=2, nodes_hi=30)
    model = gu.fill_state_(orc.SparseCADGCN(orc.Opt()), 3).double().eval()
    seen = {}
    last = model.prediction_cls[2]
    h = last.register_forward_pre_hook(lambda mod, args: seen.setdefault("c2", args[0].detach().clone()))
    d64 = yv.Data(**{k: (v.double() if v.is_floating_point() else v) for k, v in ((k, data[k]) for k in ("x", "pos", "edge", "e_attr", "bbox_idx", "bbox", "labels"))})
    with torch.no_grad():
        model(d64, slices)
    h.remove()
    lin = [m for m in last.modules() if isinstance(m, torch.nn.Linear)][0]
    return seen["c2"], lin.weight.detach(), lin.bias.detach()


def test_forward_fold_on_and_off_agree_within_twice_the_bound(forwards):
    c2, w3, b3 = _oracle_c2_w3()
    H2 = c2.shape[1]
    ref = c2 @ w3.t() + b3
    bound = ((H2 + 8) * U * (c2.abs() @ w3.abs().t()) + 2 * U * ref.abs()) * (1 + 1e-3)
    for key in forwards["on"]:
        (la, ba), (lb, bb) = forwards["on"][key], forwards["off"][key]
        assert la.shape == lb.shape == ref.shape and torch.isfinite(la).all()
        assert torch.equal(ba.view(torch.int32), bb.view(torch.int32)), ("boxes", key)
        err = (la.double() - lb.double()).abs()
        print(key, "max |on - off| / (2 bound) = %.3f" % float((err / (2 * bound)).max()))
        assert bool((err <= 2 * bound).all()), key


def test_forward_is_the_same_under_both_regimes_and_primed(forwards):
    for tag in ("on", "off"):
        first = forwards[tag]["latency_0"]
        for key, (logits, boxes) in forwards[tag].items():
            assert torch.equal(logits.view(torch.int32), first[0].view(torch.int32)), (tag, key)
            assert torch.equal(boxes.view(torch.int32), first[1].view(torch.int32)), (tag, key)
