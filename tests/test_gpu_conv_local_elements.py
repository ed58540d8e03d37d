"""GPU tests (-m gpu): the one-launch proposal-local conv stack (csrc/conv_local.hip, k_conv_local_h<NW, COO>) held per
ELEMENT to a float64 reference, one layer at a time, at the layouts that reach the limits of its tiles.

Reference: tests/conv_local_ref.py (checked on the CPU by tests/test_conv_local_ref_host.py): the header arithmetic of
conv_local.hip in float64 on the folded operands read back from the plan, layer l from the rows the kernel itself stored
for layer l - 1, with an a-priori envelope per element (half a bfloat16 spacing per storage point, carried through ReLU,
|W2f| and the mean; fp32 accumulation terms; 2^-15 |w||x| for the (hi, lo) operand pairs).  No tolerance here is a
multiple of a tensor maximum or an rms.  Beside the envelope: counting probes whose arithmetic is exact (every stored
element has ONE right bit pattern), and the e_attr (hi, lo) variant.

Every test runs on both tile shapes (NW = 4: 64 nodes / 512 edges, NW = 8: 128 / 1024) and both instantiations: the
prepared-graph (CSR) form is held to the reference, the COO form (each proposal's edges shuffled; the tile sorts them in
LDS) must be bit-identical to the CSR form of the same list.

Each envelope case prints its worst |err| / tolerance per layer (lines starting with CONV_LOCAL_RATIO; pytest -s): f over
all nodes, f_fed over the nodes with in-edges, zmean over the proposals."""
import pytest
import torch

import conv_local_ref as cl
import golden_util as gu
from conv_local_util import _run_stack, _run_stack_coo, plan_operands, to_data, tune

pytestmark = pytest.mark.gpu

L = 4
CINS = (3, 5, 8)
_MODELS = {}


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


@pytest.fixture(params=[4, 8], autouse=True)
def _waves(request):
    """both tile shapes of the kernel; the tuning goes back to automatic afterwards"""
    yield request.param
    tune(0, 0)


def _model(cin, kind=None):
    """(model, folded operands read back from its plan), built once per (in_channels, probe kind)"""
    if (cin, kind) not in _MODELS:
        yv = _yv()
        m = gu.fill_state_(yv.SparseCADGCN(yv.Opt(n_classes=17, n_blocks=L, n_blocks_out=L, in_channels=cin)), 50 + cin)
        if kind:
            cl.set_probe_state_(m, kind)
        m = m.cuda().eval().set_eval_precision("bf16")
        lay = cl.layout("ladder", 4)
        with torch.no_grad():
            m(to_data(yv, lay, *cl.inputs(lay, cin, "normal")), None)          # builds the plan: weights folded / packed
        ops = plan_operands(m._yolat_plan)
        if kind:
            cl.assert_probe_operands(ops, kind)                                 # fails, never skips
        _MODELS[(cin, kind)] = (m, ops)
    return _MODELS[(cin, kind)]


def _launch(model, lay, x, attr, NW, coo=False):
    """(feats [N, 64 L] bf16, Z_max [P, 64 L], Z_mean [P, 64 L], Z[:, :F], flag) on the CPU"""
    yv = _yv()
    tune(NW, lay["g0"])
    d = to_data(yv, lay, x, attr)
    if coo:
        feats, Z, flag, status, (F, D) = _run_stack_coo(yv, model, d, warm=False)
        assert status == 0 or flag == 1
    else:
        feats, Z, flag, (F, D) = _run_stack(yv, model, d, warm=False)
    assert D == 64 * L
    Z = Z.cpu()
    return feats.cpu(), Z[:, F:F + D], Z[:, 2 * F + D:], Z[:, :F], flag


def _both_forms(model, name, NW, cin, kind):
    """A layout in builder order on the CSR form, and with every proposal's edges shuffled on both forms; asserts what
    holds for every run (flag down, COO bit-identical to CSR, pooled max = max of the stored rows, fusion columns
    zeroed) and returns [(Csr, x, attr in CSR order, feats, Z_mean)] of the two CSR runs."""
    lay = cl.layout(name, NW)
    x, attr = cl.inputs(lay, cin, kind)
    sh, perm = cl.shuffle_inside_proposals(lay, 7)
    attr_sh = attr[torch.from_numpy(perm)].contiguous()
    out = []
    for la, at in ((lay, attr), (sh, attr_sh)):
        g = cl.Csr(la["edge"], la["bbox_idx"], la["N"], la["P"])
        feats, zmax, zmean, zf, flag = _launch(model, la, x, at, NW)
        assert flag == 0
        assert torch.equal(zmax, cl.pooled_max(feats, g)) and bool((zf == 0).all())
        out.append((g, x, at[g.perm], feats, zmean))
    feats_c, zmax_c, zmean_c, zf_c, flag = _launch(model, sh, x, attr_sh, NW, coo=True)
    assert flag == 0
    feats, zmean = out[1][3], out[1][4]
    assert torch.equal(feats_c.view(torch.int16), feats.view(torch.int16)), "COO form differs from the CSR form"
    assert torch.equal(zmax_c, cl.pooled_max(feats, out[1][0])) and torch.equal(zmean_c, zmean) and bool((zf_c == 0).all())
    return out


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("name", cl.LAYOUTS)
def test_every_stored_row_lies_inside_its_envelope(name, cin, _waves):
    """x standard normal in every column, e_attr dense of order 1: every element of every layer's stored f rows within its
    own envelope of the float64 value formed from the previous layer's stored rows; the pooled mean of the node branch
    within the envelope that travels down the s chain."""
    model, ops = _model(cin)
    pks = cl.pack_model(ops)
    for form, (g, x, attr, feats, zmean) in zip(("sorted", "shuffled"), _both_forms(model, name, _waves, cin, "normal")):
        rf = cl.check_feats(feats, x, attr, pks, g)
        rz = cl.check_zmean(zmean, x, pks, g)
        for l in range(L):
            print("CONV_LOCAL_RATIO layout=%s nw=%d cin=%d edges=%s layer=%d f=%.4f f_fed=%.4f zmean=%.4f"
                  % (name, _waves, cin, form, l, rf[l][0], rf[l][3], rz[l][0]))
        for l in range(L):
            assert rf[l][1] == 0, "f, layer %d: %d elements outside, worst |err| / tol = %.3f at (node, channel) %s" % (
                l, rf[l][1], rf[l][0], rf[l][2])
            assert rz[l][1] == 0, "mean s, layer %d: %d elements outside, worst %.3f" % (l, rz[l][1], rz[l][0])


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("name", cl.LAYOUTS)
def test_counting_probe_has_the_expected_bits(name, cin, _waves):
    """Integer codes through selector weights: f == bf16(fl32(fma(sum m, fl32(1 / deg), R))) for all 64 channels of every
    node at every layer — an edge dropped, doubled, credited to a neighbouring slot or gathered from the wrong row changes
    a code sum.  The x gather path is probed at layer 0, the e_attr path at every layer."""
    model, _ = _model(cin, "count")
    for g, x, attr, feats, _ in _both_forms(model, name, _waves, cin, "codes"):
        want = cl.count_probe_expected(x, attr, g, cin, L)
        assert cl.probe_mismatches(feats, want) == [0] * L


def test_attr_lo_halves_reach_the_stored_rows(_waves):
    """e_attr with full fp32 mantissas against small odd integer weights, in-degree 1: f == bf16(sum w attr) wherever the
    float64 value is further than 2^-16 relative from a rounding midpoint (the rest, < 2 %, is left out)."""
    model, _ = _model(5, "attr")
    for g, x, attr, feats, _ in _both_forms(model, "chain", _waves, 5, "mantissa"):
        want, keep, _ = cl.attr_probe_expected(attr, g)
        left_out = 1.0 - float(keep.double().mean())
        print("CONV_LOCAL_LEFT_OUT nw=%d share=%.5f" % (_waves, left_out))
        assert left_out <= 0.02
        assert cl.probe_mismatches(feats, want, keep) == [0] * L


@pytest.mark.parametrize("name", cl.FLAG_LAYOUTS)
def test_one_node_or_one_edge_too_many_raises_the_flag(name, _waves):
    """the exact-fit layout with T + 1 nodes, or ET + 1 edges, in its first proposal (outputs not examined)"""
    model, _ = _model(5)
    lay = cl.layout(name, _waves)
    x, attr = cl.inputs(lay, 5, "normal")
    assert _launch(model, lay, x, attr, _waves)[4] == 1
    assert _launch(model, lay, x, attr, _waves, coo=True)[4] == 1
