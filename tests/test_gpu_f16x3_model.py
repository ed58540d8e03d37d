"""GPU tests, forward level: the eval plan with its fusion launch on three half-precision products (YOLAT_FUSION_F16X3, default
on; csrc/fusion_f16x3.hip k_fusion_rows_f16x3) — a small model of cfg 2's shape (two conv layers, fusion 128 -> 1024).

  * logits with the switch on against the fp32 CPU oracle at RTOL_FWD = 1e-4 of the largest reference logit (the bar of
    tests/test_gpu_model.py), ReLU and leaky;
  * with YOLAT_FUSION_F16X3=0 the logits are bit-equal to a forward through a descriptor that carries the bf16x6 fields alone;
  * switch on, two forwards: the same bits;
  * the prepared-graph (CSR) and the COO form of one batch: bit-equal to each other.
The library reads the switch at every forward, so one process runs both forms.
"""
import ctypes
import functools

import pytest
import torch

import golden_util as gu
from oracle import oracle_torch as orc

pytestmark = pytest.mark.gpu

RTOL_FWD = 1e-4
F16_FIELDS = ("Wf_exp", "Wfs_exp")


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _optkw(act):
    return dict(n_classes=17, n_blocks=2, n_blocks_out=2, act=act)


@functools.lru_cache(maxsize=None)
def _graph():
    return _yv().synth_graph(n_classes=17, num_proposals=23, nodes_lo=3, nodes_hi=17, edge_factor=2.3, seed=61)


@functools.lru_cache(maxsize=None)
def _oracle(act):
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**_optkw(act))), 33).eval()
    with torch.no_grad():
        return ref(_graph(), None)[0]


def _model(act):
    yv = _yv()
    return gu.fill_state_(yv.SparseCADGCN(yv.Opt(**_optkw(act))), 33).cuda().eval()


def _forward_by_hand(model, desc):
    """yolat_forward_eval on `desc`, on a fresh workspace"""
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    st = model._stage_tensors(_graph())
    N, P = st["x"].shape[0], st["bbox"].shape[0]
    E, se, sc = ops.edge_layout(st["edge"])
    need = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(desc), N, E, P))
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(P, 17, device="cuda")
    check(lib.yolat_forward_eval(ctypes.byref(desc), st["x"].data_ptr(), st["x"].stride(0), st["edge"].data_ptr(), se, sc,
                                 st["e_attr"].data_ptr(), st["bbox_idx"].data_ptr(), N, E, P, out.data_ptr(), out.stride(0),
                                 ws.data_ptr(), ws.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "yolat_forward_eval")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


@pytest.mark.parametrize("act", ["relu", "leakyrelu"])
def test_switch_on_matches_the_oracle_and_switch_off_is_the_x6_forward(act, monkeypatch):
    from yolat_vectorgraphicsrecognition_amd._lib import ModelEval
    monkeypatch.delenv("YOLAT_FUSION_F16X3", raising=False)
    monkeypatch.delenv("YOLAT_STRICT_FP32", raising=False)
    model, d, want = _model(act), _graph(), _oracle(act)
    with torch.no_grad():
        on = model(d, None)[0].clone()
        on2 = model(d, None)[0].clone()
    model.check_last_status()
    desc = model._yolat_plan._desc
    assert desc.Wf_f16[0] and desc.Wf_f16[1] and desc.Wf_exp and desc.Wfs_f16[0] and desc.Wfs_f16[1] and desc.Wfs_exp
    scale = float(want.abs().max())
    err = float((on.cpu() - want).abs().max())
    print("f16x3 eval %s: %.2e of %.3g" % (act, err / scale, scale))
    assert err <= RTOL_FWD * scale
    assert torch.equal(on, on2)                                          # two forwards: the same bits
    assert torch.equal(_forward_by_hand(model, desc), on)
    # a descriptor with the bf16x6 fields alone (the f16 operands gone), switch still on ...
    x6_only = ModelEval.from_buffer_copy(desc)
    for name in F16_FIELDS:
        setattr(x6_only, name, None)
    x6_only.Wf_f16[0] = x6_only.Wf_f16[1] = x6_only.Wfs_f16[0] = x6_only.Wfs_f16[1] = None
    through_x6 = _forward_by_hand(model, x6_only)
    # ... and the full descriptor with the switch off: the same launches, the same bits
    monkeypatch.setenv("YOLAT_FUSION_F16X3", "0")
    with torch.no_grad():
        off = model(d, None)[0].clone()
    assert torch.equal(off, through_x6)
    assert torch.equal(_forward_by_hand(model, desc), through_x6)
    assert float((off.cpu() - want).abs().max()) <= RTOL_FWD * scale
    assert not torch.equal(off, on)                                      # (the switch does select another kernel)
    # the two emulations agree far inside the bar for emulated pairs (1e-5 of the logit scale)
    assert float((off - on).abs().max()) <= 1e-5 * scale


def test_prepared_graph_and_coo_forms_are_bit_equal(monkeypatch):
    monkeypatch.delenv("YOLAT_FUSION_F16X3", raising=False)
    yv = _yv()
    model, d = _model("relu"), _graph()
    with torch.no_grad():
        b, sl = yv.collate_to_device([d], csr=True)
        got_csr = model(b, sl)[0].clone()
        b2, sl2 = yv.collate_to_device([d])
        got_coo = model(b2, sl2)[0].clone()
    want = _oracle("relu")
    assert float((got_coo.cpu() - want).abs().max()) <= RTOL_FWD * float(want.abs().max())
    assert torch.equal(got_csr, got_coo)
