"""CPU tests (-m "not gpu") of the sigmoid / BCELoss entry points (csrc/loss_optim.hip) and of the BCE-head bit of the
one-call training step's descriptor (csrc/train_plan.hip): symbols and arity, argument validation before any launch, the
ABI number, and the workspace query for every value of `half`."""
import ctypes
import os
import re

import pytest

pytestmark = pytest.mark.host      # host code: CPU suite, and also the GPU box's -m gpu pass (conftest.py)

import golden_util as gu
import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"yolat_sigmoid": 7, "yolat_sigmoid_bwd": 9, "yolat_bce_work_elems": 1, "yolat_bce": 10, "yolat_sigmoid_bce": 12}


def test_the_five_symbols_are_exported_and_bound_with_matching_arity():
    src = open(os.path.join(REPO, "include", "yolat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in NAMES.items():
        assert hasattr(raw, name), "libyolat_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
        assert getattr(_lib.lib, name).argtypes is not None and len(getattr(_lib.lib, name).argtypes) == n
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m is not None, "%s is not declared in include/yolat_hip.h" % name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n
    for name in ("sigmoid", "sigmoid_bwd", "bce", "sigmoid_bce"):
        assert callable(getattr(yv.ops, name))
    assert _lib.lib.yolat_bce_work_elems(1) == 2 and _lib.lib.yolat_bce_work_elems(3000) == 13


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = _lib.lib
    one = 4096          # any non-null address: validation never dereferences
    # sigmoid(z, ldz, P, K, out, ldo, stream)
    assert lib.yolat_sigmoid(None, 17, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid(one, 17, 4, 17, None, 17, None) == -1
    assert lib.yolat_sigmoid(one, 17, 0, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid(one, 17, -3, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid(one, 17, 4, 0, one, 17, None) == -1
    assert lib.yolat_sigmoid(one, 16, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid(one, 17, 4, 17, one, 16, None) == -1
    # sigmoid_bwd(dp, lddp, p, ldp, P, K, dz, lddz, stream)
    assert lib.yolat_sigmoid_bwd(None, 17, one, 17, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, None, 17, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, one, 17, 4, 17, None, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, one, 17, 0, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, one, 17, 4, -1, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 16, one, 17, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, one, 16, 4, 17, one, 17, None) == -1
    assert lib.yolat_sigmoid_bwd(one, 17, one, 17, 4, 17, one, 16, None) == -1
    # bce(prob, ld, labels, P, K, loss, dprob, lddp, work, stream)
    assert lib.yolat_bce(None, 17, one, 4, 17, one, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 17, None, 4, 17, one, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 17, one, 4, 17, None, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 17, one, 4, 17, one, one, 17, None, None) == -1
    assert lib.yolat_bce(one, 17, one, 0, 17, one, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 17, one, 4, 0, one, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 16, one, 4, 17, one, one, 17, one, None) == -1
    assert lib.yolat_bce(one, 17, one, 4, 17, one, one, 16, one, None) == -1
    assert lib.yolat_bce(one, 17, one, 1 << 31, 17, one, None, 17, one, None) == -1
    # sigmoid_bce(logits, ld, labels, P, K, loss, dlogits, lddl, prob, ldp, work, stream)
    assert lib.yolat_sigmoid_bce(None, 17, one, 4, 17, one, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, None, 4, 17, one, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, 4, 17, None, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, 4, 17, one, one, 17, one, 17, None, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, -1, 17, one, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, 4, 0, one, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 16, one, 4, 17, one, one, 17, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, 4, 17, one, one, 16, one, 17, one, None) == -1
    assert lib.yolat_sigmoid_bce(one, 17, one, 4, 17, one, one, 17, one, 16, one, None) == -1
    with pytest.raises(_lib.YolatLibraryError):
        _lib.check(-1, "yolat_sigmoid_bce")


def test_wrappers_refuse_cpu_tensors():
    import torch
    z, y, loss = torch.zeros(4, 17), torch.zeros(4, dtype=torch.int64), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.sigmoid(z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.sigmoid_bwd(z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.bce(z, y, loss)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yv.ops.sigmoid_bce(z, y, loss)


def test_abi_version_is_unchanged():
    assert _lib.lib.yolat_abi_version() == 6


# yolat_train_step_workspace_bytes(N = 20000, E = 40000, P = 800) of the "small" fixture model before the BCE head existed
# (half = 0 / 1 / 3), recorded from that build: the new bit must not move a byte of the softmax model's workspace
WS_BEFORE = {0: 335803648, 1: 305083648, 3: 318895104}


def test_train_step_workspace_for_every_half_value():
    """half = 0 / 1 / 3 (fp32 / bf16 / bf16_dense, softmax head): the workspace is what it was; bit 4 (the BCE head) on top
    of each is accepted and sized — the loss scratch is the larger of the two losses', the same element count here —
    and bits above it are refused."""
    _, optkw = gu.graph_case("small")
    opt = yv.Opt(**optkw)
    tr = yv.Trainer(yv.SparseCADGCN(opt), opt)
    assert tr.plan.prepare()
    d = tr.plan._desc
    q = lambda: int(_lib.lib.yolat_train_step_workspace_bytes(ctypes.byref(d), 20000, 40000, 800))
    need = {}
    for half in (0, 1, 3, 4, 5, 7):
        d.half = half
        need[half] = q()
        assert need[half] > 0, half
    for half, want in WS_BEFORE.items():
        assert need[half] == want, (half, need[half], want)
    assert (need[4], need[5], need[7]) == (need[0], need[1], need[3])
    for half in (8, 12, 16, -1):
        d.half = half
        assert q() == 0, half


def test_trainer_sets_the_bce_bit_for_a_sigmoid_model_and_keeps_the_defaults():
    _, optkw = gu.graph_case("small")
    for classifier, bit in (("softmax", 0), ("sigmoid", 4)):
        opt = yv.Opt(**dict(optkw, classifier=classifier))
        model = yv.SparseCADGCN(opt)
        tr = yv.Trainer(model, opt)
        assert tr.plan.model_fits()
        for prec, half in (("fp32", 0), ("bf16", 1), ("bf16_dense", 3)):
            model.set_train_precision(prec)
            assert tr.plan.prepare() and tr.plan._desc.half == (half | bit)
    # everything else the plan declines stays declined
    opt = yv.Opt(**dict(optkw, classifier="sigmoid", dropout=0.3))
    assert not yv.Trainer(yv.SparseCADGCN(opt), opt).plan.model_fits()
