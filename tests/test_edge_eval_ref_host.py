"""The helpers of tests/edge_eval_ref.py are what they claim to be (no GPU needed): the graph table reaches the tiles,
passes and chunks it was written for (restated host formulas), the float64 reference is the oracle's conv layer in double
and its two argument forms agree, the inputs are full-mantissa fp32 with the stated special columns, and — the proof that
tests/test_gpu_edge_eval_elements.py can fail for a subtly wrong kernel — every envelope accepts its defect-free fp32
emulation on every graph of the table and rejects each planted defect on the graphs named for it."""
import functools

import numpy as np
import pytest
import torch

import bf16_ref as br
import edge_eval_ref as er
import golden_util as gu
from oracle import oracle_torch as orc

pytestmark = pytest.mark.host

REJECT_GRAPHS = ["ladder", "hub150", "hub1000"]
# the two 12 000-node graphs only move the chained kernel's chunk from one to two and three 16-edge steps, which no
# emulation models (they walk rows, not streams): a CPU run of them would cost seconds and show nothing the other graphs
# do not.  The bf16 envelopes are accepted on every other graph of the table.
BF16_HOST_GRAPHS = er.FP32_GRAPHS


def _inside(got, want, tol):
    """(all inside, worst |err| / tol); NaN counts as outside"""
    got = torch.as_tensor(np.asarray(got)).double() if not torch.is_tensor(got) else got.double()
    err = (got - want).abs()
    ok = err <= tol
    r = err / tol.clamp_min(1e-300)
    r = torch.where(torch.isfinite(r) | (err == 0), r, torch.full_like(r, float("inf")))
    return bool(ok.all()), (float(r.max()) if r.numel() else 0.0)


@functools.lru_cache(maxsize=None)
def _case(name, bf16=False):
    """(N, E, src, dst numpy CSR, row_ptr, inputs, CSR attr, src, dst tensors) of a table graph"""
    N, E, s, d, order, ptr = er.csr_case(name)
    inp = er.stage_inputs_bf16(N, E, N + E) if bf16 else er.stage_inputs(N, E, N + E)
    attr = inp["attr"][torch.from_numpy(order)]
    return N, E, s, d, ptr, inp, attr, torch.from_numpy(s), torch.from_numpy(d)


def _layout(E, N, kind):
    """the pass structure an emulation walks: "tiles" the node tiles, "ws" the 64-row passes of the wave-specialised
    kernel's chunks (tiles below one full pass), "chain" the 16-row steps of the chained kernel's chunks"""
    if kind == "ws" and E >= 64:
        return ("ws", er.ws_layout(E)["chunk"], er.PASS)
    if kind == "chain" and E >= 16:
        return ("ws", er.chain_layout(E)["chunk"], 16)
    return ("tiles", er.edge_tile_npt(N, E), er.PASS)


# ---------------------------------------------------------------------------------------------
# generators and the table
# ---------------------------------------------------------------------------------------------
def test_gaps_has_the_stated_empty_nodes():
    src, dst = er.gaps()
    assert src.dtype == dst.dtype == np.int64 and len(src) == len(dst) == 90
    deg = np.bincount(dst, minlength=200)
    assert not deg[:70].any() and not deg[130:].any()
    assert int((deg[70:130] == 0).sum()) == 10 and int((deg[70:130] > 0).sum()) == 50
    assert (np.diff(dst) < 0).any()
    a, b = er.gaps()
    assert np.array_equal(a, src) and np.array_equal(b, dst)


@pytest.mark.parametrize("name", list(er.EDGE_GRAPHS))
def test_table_entry_reaches_what_it_was_written_for(name):
    """npt, NG, tiles, the ws chunk and grid and the chained kernel's chunk of every entry, from the restated host
    formulas, against the literal numbers of EXPECT — and the structural facts the table's comments name"""
    N, E, s, d, order, ptr = er.csr_case(name)
    tl, ws, ch = er.tile_layout(N, E), er.ws_layout(E), er.chain_layout(E)
    assert (N, E, tl["npt"], tl["NG"], tl["tiles"], ws and ws["chunk"], ws and ws["grid"], ch and ch["chunk"]) == er.EXPECT[name]
    deg = np.diff(ptr)
    if name == "ladder":
        assert sorted(deg[:41].tolist()) == list(range(41)) and N % tl["npt"] == 0 and E % 64 == 52
        per_tile = [int(ptr[min(N, n + 3)] - ptr[n]) for n in range(0, N, 3)]
        assert any(0 < e <= 64 for e in per_tile) and any(64 < e <= 128 for e in per_tile)
    if name.startswith("hub") and N == 300:
        hub = int(name[3:])
        b, e = int(ptr[br.HUB_IN]), int(ptr[br.HUB_IN + 1])
        assert e - b == hub
        ranges = er.pass_ranges(ptr, d, N, E, ("ws", 64, 64))
        eS = [r[0] for r in ranges if r[0] <= b < r[1]][0]             # the range that owns the hub walks it from eS
        assert (e - 1 - eS) // 64 - (b - eS) // 64 + 1 >= {65: 2, 150: 3, 1000: 16}[hub]
        inside = [c for c in range(64, E, 64) if b < c and c + 64 <= e]     # ws chunks wholly inside the hub: no range
        assert len(inside) >= {65: 0, 150: 1, 1000: 14}[hub] and len(ranges) <= ws["grid"] - len(inside)
    if name == "chain257":
        assert (deg == 1).all() and N - 4 * tl["npt"] == 33
    if name == "tiny":
        assert tl["tiles"] == 1 and ws is None and ch is None
    if name.startswith("u50_") and E > 64:
        assert d[63] == d[64]                       # the chunk boundary at row 64 falls inside a node
    if name == "u50_65":
        assert len(er.pass_ranges(ptr, d, N, E, ("ws", 64, 64))) == 1      # ... so the second workgroup has no range
    if name in ("u4000_32769", "hub4000_65537"):
        assert ws["chunk"] // 64 == (2 if E == 32769 else 3)
        assert er.ws_layout(E - 1)["chunk"] // 64 == (1 if E == 32769 else 2)
    if name in er.BF16_ONLY:
        assert ch["chunk"] // 16 == (2 if E == 98305 else 3)
        assert er.chain_layout(E - 1)["chunk"] // 16 == (1 if E == 98305 else 2)


def test_dispatch_thresholds_of_the_restated_formulas():
    assert er.tile_layout(160, 560)["NG"] == 1 and er.tile_layout(170, 560)["NG"] == 4
    assert er.ws_layout(63) is None and er.ws_layout(64) == dict(chunk=64, grid=1)
    assert er.chain_layout(15) is None and er.chain_layout(16) == dict(chunk=16, grid=1)
    assert er.edge_tile_npt(10, 0) == 64 and er.edge_tile_npt(1, 1000) == 1


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "tiny"])
def test_reference_is_the_oracle_conv_layer_in_double_and_its_two_forms_agree(name):
    """oracle.AttrRelativeEdgeConvGlobalPool2 in eval mode, run in double, against edge_stage_ref on the factorised
    operands (UV = x . [W1a - W1b | W1b]^T, the attr columns, the folded BatchNorms as (s, t)) — unfolded, and folded by
    the product's own ops.fold_factorised_layer, in float64"""
    N, E, s, d, order, ptr = er.csr_case(name)
    conv = gu.fill_state_(orc.AttrRelativeEdgeConvGlobalPool2(64, 64), 5).double().eval()
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, 64, generator=g, dtype=torch.float64)
    attr = torch.randn(E, 4, generator=g, dtype=torch.float64)
    st, dt = torch.from_numpy(s), torch.from_numpy(d)
    with torch.no_grad():
        want, _ = conv(x, torch.relu(x), torch.stack([st, dt]), None, attr)

    def folded(bn):
        sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return sc.detach(), (bn.bias - bn.running_mean * sc).detach()
    W1 = conv.nn[0].weight.detach()
    wuv = torch.cat([W1[:, :64] - W1[:, 64:128], W1[:, 64:128]])
    wc4 = W1[:, 128:132].contiguous()
    (s1, t1), (s2, t2) = folded(conv.nn[1]), folded(conv.nn[4])
    b1, b2 = conv.nn[0].bias.detach(), conv.nn[3].bias.detach()
    root = (x @ conv.lin_r.weight.t() + conv.lin_r.bias).detach()
    inp = dict(UV=x @ wuv.t(), wc4=wc4, b1=b1, s1=s1, t1=t1, W2=conv.nn[3].weight.detach(), b2=b2, s2=s2, t2=t2, root=root)
    ref = er.edge_stage_ref(inp, st, dt, attr, N)
    assert float((ref["out"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    from yolat_vectorgraphicsrecognition_amd import ops
    wuvf, uvb, wc4f, t2f = ops.fold_factorised_layer(wuv, wc4, b1, s1, t1, b2, s2, t2)
    inf = dict(UV=x @ wuvf.t() + uvb, wc4=wc4f, b1=None, s1=None, t1=None, W2=inp["W2"], b2=None, s2=s2, t2=t2f, root=root)
    for x6 in (False, True):
        rf = er.edge_stage_ref(inf, st, dt, attr, N, x6=x6)
        assert float((rf["out"] - ref["out"]).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float((rf["m"] - ref["m"]).abs().max()) <= 1e-12 * float(ref["m"].abs().max())
    # the helper's own fold is that fold
    f2 = er.fold_inputs(inp)
    assert torch.allclose(f2["UV"], inf["UV"], rtol=0, atol=1e-13) and torch.equal(f2["wc4"], wc4f) and torch.equal(f2["t2"], t2f)


def test_mean_tol_holds_the_run_sum_term():
    mag, deg = torch.tensor([[3.0], [7.0]], dtype=torch.float64), torch.tensor([[5.0], [1000.0]], dtype=torch.float64)
    assert torch.allclose(er.mean_tol(mag, deg), er.run_sum_tol(mag, deg) / deg + er.U * mag / deg, rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def test_inputs_are_full_mantissa_with_the_stated_special_columns():
    inp = er.stage_inputs(300, 2000, 7)
    for k in ("UV", "attr", "wc4", "b1", "s1", "t1", "W2", "b2", "s2", "t2", "root"):
        assert inp[k].dtype == torch.float32 and er.has_full_mantissa(inp[k]), k
    assert int((inp["s2"] < 0).sum()) == 16 and bool((inp["s2"].abs() >= 0.5).all())
    assert bool((inp["t2"][list(er.CLOSED)] == -50).all()) and int((inp["t2"] == -50).sum()) == 2
    assert bool((inp["W2"][:, er.ZERO_K] == 0).all()) and int((inp["W2"] == 0).sum()) == 64
    fo = er.fold_inputs(inp)
    for k in ("UV", "wc4", "t2"):
        assert fo[k].dtype == torch.float32 and er.has_full_mantissa(fo[k]), k
    assert fo["b1"] is None and fo["s1"] is None and fo["t1"] is None and fo["b2"] is None
    assert bool((fo["t2"][list(er.CLOSED)] < -49).all())
    h = er.stage_inputs_bf16(300, 2000, 7)
    assert h["UV"].dtype == h["W2f"].dtype == torch.bfloat16 and er.has_full_mantissa(h["root"])
    assert bool((h["W2f"][:, er.ZERO_K] == 0).all()) and bool((h["t2f"][list(er.CLOSED)] == -50).all())


@pytest.mark.parametrize("name", ["ladder", "hub1000", "gaps"])
def test_closed_columns_and_empty_nodes_are_the_root_in_reference_and_emulation(name):
    N, E, s, d, ptr, inp, attr, st, dt = _case(name)
    for ip in (inp, er.fold_inputs(inp)):
        for x6 in (False, True):
            ref = er.edge_stage_ref(ip, st, dt, attr, N, x6=x6)
            got = er.emulate_stage(ip, s, d, attr, ptr, N, _layout(E, N, "ws"), x6=x6)
            cl = list(er.CLOSED)
            assert bool((ref["m"][:, cl] == 0).all()) and torch.equal(ref["out"][:, cl], ip["root"].double()[:, cl])
            assert np.array_equal(got[:, cl], ip["root"].numpy()[:, cl])
            empty = np.diff(ptr) == 0
            assert empty.any() and np.array_equal(got[empty], ip["root"].numpy()[empty])
            assert bool((ref["tol"][torch.from_numpy(empty)] == 0).all())


# ---------------------------------------------------------------------------------------------
# the envelopes accept the clean emulations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x6", [False, True])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", er.FP32_GRAPHS)
def test_fp32_envelopes_accept_the_clean_emulation(name, fold, x6):
    """messages and outputs, per element; the emulation walks the node tiles for the fp32-MFMA forms and the ws chunks
    for X6, and both walks return the same bits"""
    N, E, s, d, ptr, inp, attr, st, dt = _case(name)
    ip = er.fold_inputs(inp) if fold else inp
    ref = er.edge_stage_ref(ip, st, dt, attr, N, x6=x6)
    msg = er.emulate_messages(ip, s, d, attr, x6=x6)
    ok, r = _inside(msg, ref["m"], ref["tol_m"])
    assert ok, "messages: worst error / tolerance %.3f" % r
    root = ip["root"].numpy()
    got = er.emulate_aggregate(msg, ptr, root, N, _layout(E, N, "ws" if x6 else "tiles"))
    ok, r = _inside(got, ref["out"], ref["tol"])
    print("ratio %-14s fold=%d x6=%d %.3f" % (name, fold, x6, r))
    assert ok, "outputs: worst error / tolerance %.3f" % r
    if E <= 2000:
        other = er.emulate_aggregate(msg, ptr, root, N, _layout(E, N, "tiles" if x6 else "ws"))
        assert np.array_equal(got.view(np.int32), other.view(np.int32))


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("name", BF16_HOST_GRAPHS)
def test_bf16_envelope_accepts_the_clean_emulation_and_the_flip_allowance_does_not_carry_it(name, chain):
    """No output of the clean emulation leaves the derived bound, and the bound is not the flip allowance: the median
    over the outputs of the flip term is <= the median of the base term (store half-spacing + fp32 noise).  Prints the
    flagged share of the hidden activations (measured here with the input scales of tests/test_gpu_bf16.py, Wc4 ~ 2 N(0,
    1): at most 0.22 % for the node tiles, 1.2-1.6 % for the chained kernel, whose 2^-16 attr term widens dz)."""
    N, E, s, d, ptr, inp, attr, st, dt = _case(name, True)
    ref = er.edge_stage_ref_bf16(inp, st, dt, attr, N, chain)
    print("flagged %-14s chain=%d share %.4f  median flip %.3e  median base %.3e" % (
        name, chain, ref["flagged"], float(ref["flip"].median()), float(ref["base"].median())))
    assert float(ref["flip"].median()) <= float(ref["base"].median())
    assert ref["flagged"] <= 0.03
    if chain and E < 16:
        return
    got = er.emulate_stage_bf16(inp, s, d, attr, ptr, N, _layout(E, N, "chain" if chain else "tiles"), chain)
    ok, r = _inside(got, ref["out"], ref["tol"])
    assert ok, "worst error / tolerance %.3f" % r
    empty = torch.from_numpy(np.diff(ptr) == 0)
    assert torch.equal(got[empty], inp["root"][empty].to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------
# the envelopes reject the planted defects
# ---------------------------------------------------------------------------------------------
# A defect that cannot fire on a graph returns the clean bits; these are all such pairs (checked both ways below):
#   stale_root    no aggregation thread finishes two nodes in a pass: a pass (a tile) of these graphs holds <= 16 nodes
#   carry_lost    the ladder's longest run, 40 rows, spans at most two 64-row passes (three of the chained kernel's 16)
#   chunk_overlap the node tiles have no chunks
def _unreached(defect, name, walk):
    if defect == "stale_root":
        return name in REJECT_GRAPHS or walk == "chain"
    if defect == "carry_lost":
        return (name == "ladder" and walk != "chain") or name in ("chain257", "gaps") or (name == "u50_65" and walk != "chain")
    if defect == "chunk_overlap":
        return walk == "tiles" or name in ("chain257",) or (name == "gaps" and walk != "chain")
    if defect in ("boundary_twice", "pass_count"):
        return name == "chain257" or (name in ("gaps", "u50_65") and walk != "chain")
    if defect == "deg0_unwritten":
        return name == "chain257"
    return False


REJECT_CASES = [(n, df) for n in REJECT_GRAPHS for df in er.AGG_DEFECTS] + [("chain257", "stale_root"), ("u50_65", "chunk_overlap")]


@pytest.mark.parametrize("x6", [False, True])
@pytest.mark.parametrize("name,defect", REJECT_CASES + [(n, df) for n in REJECT_GRAPHS for df in er.MSG_DEFECTS_X6])
def test_fp32_envelopes_reject_the_planted_defects(name, defect, x6):
    """unfolded operands through the fp32-MFMA arithmetic, folded through X6, both walked as ws chunks"""
    if defect in er.MSG_DEFECTS_X6 and not x6:
        return
    N, E, s, d, ptr, inp, attr, st, dt = _case(name)
    ip = er.fold_inputs(inp) if x6 else inp
    ref = er.edge_stage_ref(ip, st, dt, attr, N, x6=x6)
    lay = _layout(E, N, "ws")
    clean = er.emulate_stage(ip, s, d, attr, ptr, N, lay, x6=x6)
    got = er.emulate_stage(ip, s, d, attr, ptr, N, lay, x6=x6, defect=defect)
    same = np.array_equal(got.view(np.int32), clean.view(np.int32))
    assert same == _unreached(defect, name, "ws"), "%s on %s: reach" % (defect, name)
    ok, r = _inside(got, ref["out"], ref["tol"])
    assert ok == same, "%s on %s: worst error / tolerance %.3f" % (defect, name, r)


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("name,defect", REJECT_CASES + [(n, df) for n in REJECT_GRAPHS for df in er.BF16_DEFECTS]
                         + [("gaps", "deg0_unwritten")])
def test_bf16_envelope_rejects_the_planted_defects(name, defect, chain):
    """the node-tile arithmetic walked as node tiles, the chained kernel's walked as its chunks in 16-row steps"""
    N, E, s, d, ptr, inp, attr, st, dt = _case(name, True)
    walk = "chain" if chain else "tiles"
    ref = er.edge_stage_ref_bf16(inp, st, dt, attr, N, chain)
    lay = _layout(E, N, walk)
    clean = er.emulate_stage_bf16(inp, s, d, attr, ptr, N, lay, chain)
    got = er.emulate_stage_bf16(inp, s, d, attr, ptr, N, lay, chain, defect=defect)
    same = torch.equal(got.view(torch.int16), clean.view(torch.int16))
    assert same == _unreached(defect, name, walk), "%s on %s: reach" % (defect, name)
    ok, r = _inside(got, ref["out"], ref["tol"])
    assert ok == same, "%s on %s: worst error / tolerance %.3f" % (defect, name, r)


@pytest.mark.parametrize("name", REJECT_GRAPHS)
def test_x6_low_terms_alone_measured(name):
    """Dropping ONLY a_h b_l and a_l b_h of the X6 split costs about 2^-16 per product with random sign — it was expected to
    hide below a worst-case 64-term bound, and the bound is not bent to catch it.  Measured on the folded operands: it IS
    caught on all three graphs, worst error / tolerance 2.9 (ladder), 2.7 (hub150), 3.6 (hub1000) against 0.02 for the
    clean emulation — the envelope is driven by layer 1's and the run sum's terms at typical magnitudes, not by 64 worst-
    case roundings at the operands' maxima.  Asserted here only as a record of the margin: > 1, and < 10, i.e. a defect of
    2^-18 per product would pass."""
    N, E, s, d, ptr, inp, attr, st, dt = _case(name)
    ip = er.fold_inputs(inp)
    ref = er.edge_stage_ref(ip, st, dt, attr, N, x6=True)
    got = er.emulate_stage(ip, s, d, attr, ptr, N, _layout(E, N, "ws"), x6=True, defect="no_l_terms")
    ok, r = _inside(got, ref["out"], ref["tol"])
    print("ratio no_l_terms %-8s %.3f" % (name, r))
    assert not ok and 1.0 < r < 10.0
