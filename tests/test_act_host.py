"""CPU tests (-m "not gpu") of the leakyrelu / prelu surface (torch_nn.py:9-20, config.py --act): module types, state_dict
keys against the oracle's, ABI symbols, what declines, and the flat parameter layout."""
import ctypes

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.host

import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import _lib, engine, nn_modules, trainer
from oracle import oracle_torch as orc

SLOPE_KEYS = ["cls_net.fusion_block.2.weight", "cls_net.fusion_block_super.2.weight", "prediction_cls.0.2.weight",
              "prediction_cls.1.2.weight"]


def test_act_layer_returns_the_reference_modules():
    assert isinstance(nn_modules.act_layer("relu"), nn.ReLU)
    lk = nn_modules.act_layer("LeakyReLU")
    assert isinstance(lk, nn.LeakyReLU) and lk.negative_slope == 0.2
    pr = nn_modules.act_layer("prelu")
    assert isinstance(pr, nn.PReLU) and pr.weight.shape == (1,) and float(pr.weight.detach()) == pytest.approx(0.2)
    with pytest.raises(ValueError, match="n_prelu"):
        nn_modules.act_layer("prelu", n_prelu=4)
    with pytest.raises(NotImplementedError, match="is not found"):
        nn_modules.act_layer("swish")


@pytest.mark.parametrize("act", ["leakyrelu", "prelu"])
def test_state_dict_keys_equal_the_oracles(act):
    m = yv.SparseCADGCN(yv.Opt(act=act))
    r = orc.SparseCADGCN(orc.Opt(act=act))
    got, want = m.state_dict(), r.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in got:
        assert got[k].shape == want[k].shape, k
    extra = [k for k in got if k not in yv.SparseCADGCN(yv.Opt()).state_dict()]
    assert extra == (SLOPE_KEYS if act == "prelu" else [])
    # the conv layers' own MLPs stay ReLU (torch_vertex.py:309-311)
    for cv in engine.model_convs(m.cls_net):
        assert isinstance(cv.nn[2], nn.ReLU) and isinstance(cv.mlp_node[2], nn.ReLU)
    kinds = engine.model_act(m)
    assert all(isinstance(a, nn.PReLU if act == "prelu" else nn.LeakyReLU) for a in kinds)


def test_reference_prelu_checkpoint_loads_strictly():
    r = orc.SparseCADGCN(orc.Opt(act="prelu"))
    with torch.no_grad():
        for i, k in enumerate(SLOPE_KEYS):
            r.state_dict()[k].fill_(-0.3 + 0.25 * i)
    m = yv.SparseCADGCN(yv.Opt(act="prelu"))
    epoch, best = trainer.load_reference_checkpoint(m, {"epoch": 3, "state_dict": {"module." + k: v for k, v in
                                                                                   r.state_dict().items()},
                                                        "best_value": 0.5}, strict=True)
    assert (epoch, best) == (3, 0.5)
    for i, k in enumerate(SLOPE_KEYS):
        assert float(m.state_dict()[k]) == pytest.approx(-0.3 + 0.25 * i)
    with pytest.raises(RuntimeError):
        trainer.load_reference_checkpoint(yv.SparseCADGCN(yv.Opt()), {"state_dict": r.state_dict()}, strict=True)


def test_new_abi_symbols_exist():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yolat_scale_shift_act", "yolat_segment_act_max", "yolat_bn_act_bwd", "yolat_bn_act_bwd_work_elems",
                 "yolat_fusion_pair_eval_act", "yolat_fusion_pair_eval_act_work_elems", "yolat_fusion_pair_eval_x6_act",
                 "yolat_pool_init_signed"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    names = [f[0] for f in _lib.ModelEval._fields_]
    assert "act" in names and "act_slope" in names and "reserved" not in names
    assert _lib.ModelEval.act.offset == 12 and _lib.ModelEval.C.offset == 16      # the former `reserved` word
    assert _lib.lib.yolat_bn_act_bwd_work_elems(300, 70) == 3 * 2 * 70 + 3 * 70
    # argument validation happens before any launch
    assert _lib.lib.yolat_scale_shift_act(None, 4, 3, 4, None, None, None, None, 4, None) == -1


@pytest.mark.parametrize("act", ["leakyrelu", "prelu"])
def test_modes_without_a_leaky_kernel_decline_loudly(act):
    m = yv.SparseCADGCN(yv.Opt(act=act))
    with pytest.raises(ValueError, match="act"):
        m.set_eval_precision("bf16")
    with pytest.raises(ValueError, match="act"):
        m.set_train_precision("bf16")
    with pytest.raises(ValueError, match="act"):
        m.set_train_precision("bf16_dense")
    m.set_eval_precision("fp32")
    m.set_train_precision("fp32")

    class _T(object):
        model = m
    assert trainer.TrainPlan(_T()).model_fits() is False
    _T.model = yv.SparseCADGCN(yv.Opt())
    assert trainer.TrainPlan(_T()).model_fits() is True
    with pytest.raises(NotImplementedError):
        yv.SparseCADGCN(yv.Opt(act=act, norm="layer"))


def _offsets(model):
    flat = trainer.FlatParams(model)
    base = flat.param.data_ptr()
    return flat, [(p.data_ptr() - base) // 4 for p in flat.params]


def test_flat_params_keep_every_view_16_byte_aligned():
    m = yv.SparseCADGCN(yv.Opt(act="prelu"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flat, offs = _offsets(m)
    assert offs == flat.offsets
    slope_ids = {id(mod.weight) for mod in m.modules() if isinstance(mod, nn.PReLU)}
    assert len(slope_ids) == 4
    for p, off in zip(flat.params, offs):
        assert off % 4 == 0 and p.data_ptr() % 16 == 0
        assert flat.grad_views[id(p)].data_ptr() % 16 == 0
    # values survive, the padding is zero and belongs to no parameter
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    covered = torch.zeros(flat.numel, dtype=torch.bool)
    for p, off in zip(flat.params, offs):
        covered[off:off + p.numel()] = True
    assert int((~covered).sum()) == 4 * 3 and float(flat.param[~covered].abs().max()) == 0.0
    assert float(flat.grad.abs().max()) == 0.0
    # Adam's torch-format state speaks per parameter, padding excluded
    opt = trainer.FlatAdam(flat)
    opt.step_count = 1
    sd = opt.state_dict()
    assert [tuple(sd["state"][i]["exp_avg"].shape) for i in range(len(flat.params))] == [tuple(p.shape) for p in flat.params]
    opt.load_state_dict(sd)


@pytest.mark.parametrize("act", ["relu", "leakyrelu"])
def test_flat_params_of_a_model_without_slopes_are_back_to_back(act):
    m = yv.SparseCADGCN(yv.Opt(act=act, n_classes=22))
    flat, offs = _offsets(m)
    want, n = [], 0
    for p in m.parameters():
        want.append(n)
        n += p.numel()
    assert offs == want and flat.numel == n
