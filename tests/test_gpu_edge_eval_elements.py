"""GPU tests (-m gpu) of the fused EVAL edge stage — factorised edge MLP, mean aggregation, root row — per element against
float64 references with derived bounds (tests/edge_eval_ref.py; tests/test_edge_eval_ref_host.py shows on the CPU that
every bound accepts an fp32 emulation of the kernels and rejects a dropped or doubled row, a lost carry, a wrong divisor, a
stale or missing root row, a node summed by two workgroups, missing terms of the X6 split, a truncated h1 and an unwritten
node).  fp32: k_edge_uv_mlp2_mean<1|4>, k_edge_mt_uv_mlp2_mean, k_edge_uv_mlp2_mean_ws<FOLD, X6> and the message kernel
k_edge_uv_mlp2 (csrc/edge.hip); bf16 storage: k_edge_uv_mlp2_mean_h<1|4> and k_edge_chain_h (csrc/edge_chain.hip).

Graphs: edge_eval_ref.EDGE_GRAPHS — the ladder, the hubs over 2, 3 and 16 passes, the chain, 7 edges, `gaps` (70 empty nodes
in front and behind), E = 63 .. 129 over 50 nodes, the NG = 1 / NG = 4 dispatch edge, and the smallest E at which a
wave-specialised workgroup owns two and three passes (bf16: a stream of the chained kernel two and three steps).

Conventions (those of test_gpu_fp32_graph_ops.py): operands and outputs are column slots of wider NaN-filled buffers (f_out
= columns 64:128 of [N + 3, 128]; UV with a row stride of 132 floats on the ladder, 136 bf16 values in the bf16 test);
everything outside the output slot keeps its bits; each call runs twice with equal bits; the float64 references are
evaluated on the device; each check prints its worst error / tolerance.  No tolerance is scaled by a tensor maximum and no
share of the outputs is exempt.

Largest error / envelope seen on the MI355X, per kernel and route (all graphs, both argument forms):
  fp32, worst over the 17 graphs and both forms (the envelope charges each of layer 2's 64 terms a full rounding at
  |h1| |W2| and layer 1's six roundings at the magnitude sum; the kernels' errors are random in sign, so all sit far below 1
  — what the bound still rejects is shown on the CPU, down to an X6 split without its a_h b_l and a_l b_h terms at 2.7-3.6):
    TILES = MT2 = MT3 = MT16 = WS_F32 (the same bits)   0.046   chain257, folded
    WS_X6                                               0.038   uniform(50, 65), folded;  AUTO at E = 131072: 0.037
    messages (k_edge_uv_mlp2)                           0.051   ladder, folded
  bf16, worst over the 19 graphs:
    node tiles 1.000, chained 1.000 — by construction, not by the kernels: the store's half spacing leads the bound, and a
    node without in-edges holds bf(root) with no other term.  The element: hub65, node 172 (no in-edge), column 19, whose
    fp32 root ends in the bits 0x7fff, one fp32 step below a bf16 midpoint: error / bound = 1 - 2^-15 for ANY correct
    store, the CPU emulation included.
    outputs beyond the base term (store half spacing + fp32 noise), i.e. carried by the derived flip allowance: node tiles
    75 of 2 179 328 (worst error / base 4.6), chained 3 747 of 2 181 248 (worst 18.4, where root and mean cancel); none
    beyond the bound.  Flagged hidden activations: at most 0.22 % (node tiles), 1.2-1.4 % (chained, whose 2^-16 attr term
    widens dz).
"""
import functools
import os

import numpy as np
import pytest
import torch

import edge_eval_ref as er

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
NAN = float("nan")
TILES, WS_F32, WS_X6 = 1, 2, 3


def _ops():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv.ops


def _lib():
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    return lib, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _worst(op, name, got, want, tol):
    """asserts |got - want| <= tol (elementwise, NaN fails); prints and returns the worst error / tolerance"""
    err = (got.double() - want).abs()
    ok = err <= tol
    r = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    ratio = float(r.max()) if err.numel() else 0.0
    print("ratio %-26s %-16s %.3f" % (op, name, ratio))
    assert bool(ok.all()), "%s %s: %d of %d outside the tolerance, worst error / tolerance %.3f" % (
        op, name, int((~ok).sum()), ok.numel(), ratio)
    return ratio


def _slot(rows, width, lo, hi, dtype=F32):
    """(view [rows, hi - lo], buffer [rows + 3, width]) of a NaN-filled buffer"""
    buf = torch.full((rows + 3, width), NAN, dtype=dtype, device=DEV)
    return buf[:rows, lo:hi], buf


def _outside_untouched(buf, snap, rows, lo, hi):
    """everything outside the slot [:rows, lo:hi] holds the bits of the snapshot"""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[:rows, lo:hi] = False
    return torch.equal(_bits(buf)[mask], _bits(snap)[mask])


def _build(N, src, dst, attr):
    """ops.Graph of the edge LIST (src, dst, attr in list order), checked against the numpy CSR; returns (graph, CSR
    src, dst int64 device tensors, CSR attr, row_ptr numpy)"""
    ops = _ops()
    E = len(src)
    g = ops.build_graph(torch.from_numpy(np.stack([src, dst], 1)).to(DEV), attr.to(DEV), None, N, 1)
    g.check_status()
    order, row_ptr, _, _ = er.csr_of(src, dst, N)
    s, d = (torch.from_numpy(np.ascontiguousarray(x[order])).to(DEV) for x in (src, dst))
    a = attr[torch.from_numpy(order)].to(DEV)
    assert torch.equal(g.src[:E].long(), s) and torch.equal(g.dst[:E].long(), d) and torch.equal(g.attr[:E], a)
    assert torch.equal(g.row_ptr.long().cpu(), torch.from_numpy(row_ptr))
    return g, s, d, a, row_ptr


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(N, E, graph, s, d, attr, row_ptr) of a table graph; the attr are those of stage_inputs / stage_inputs_bf16 (the
    same draws)"""
    N, src, dst = er.EDGE_GRAPHS[name]()
    E = len(src)
    attr = er.randn32((max(E, 1), 4), N + E + 1, 0.5)[:E]
    return (N, E) + _build(N, src, dst, attr)


def _dev(inp):
    return {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}


def _twice(run):
    a, b = run(), run()
    assert torch.equal(_bits(a), _bits(b))
    return a


# ---------------------------------------------------------------------------------------------
# fp32 stage
# ---------------------------------------------------------------------------------------------
def _fp32_operands(name, N, E, fold, ld_uv):
    inp = er.stage_inputs(N, E, N + E)
    inp = _dev(er.fold_inputs(inp) if fold else inp)
    uv, uvbuf = _slot(N, ld_uv, 0, 128)
    uv.copy_(inp["UV"])
    inp["UV"] = uv
    return inp, uvbuf


def _run_fp32(inp, g, N, route):
    """f_out [N,64] of one route: ("v", variant) or ("mt", tiles_per_wg); f_out pre-loaded with root, twice, the same
    bits, nothing outside the slot touched"""
    ops = _ops()
    fo, fbuf = _slot(N, 128, 64, 128)
    p1 = (inp["s1"], inp["t1"]) if inp["s1"] is not None else None

    def run():
        fo.copy_(inp["root"])
        snap = fbuf.clone()
        if route[0] == "v":
            ops.edge_uv_mlp2_mean_eval(inp["UV"], g, inp["wc4"], inp["b1"], p1, inp["W2"], inp["b2"], (inp["s2"], inp["t2"]),
                                       fo, variant=route[1])
        else:
            ops.edge_uv_mlp2_mean_eval_mt(inp["UV"], g, inp["wc4"], inp["b1"], p1, inp["W2"], inp["b2"],
                                          (inp["s2"], inp["t2"]), fo, tiles_per_wg=route[1])
        assert _outside_untouched(fbuf, snap, N, 64, 128)
        return fo.clone()
    return _twice(run)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", er.FP32_GRAPHS)
def test_edge_stage_fp32_every_route_matches_fp64_per_element(name, fold):
    """ops.edge_uv_mlp2_mean_eval(variant = 1, 2, 3) and ops.edge_uv_mlp2_mean_eval_mt(tiles_per_wg = 2, 3, 16) on every
    table graph, unfolded and folded.  (a) every route inside its envelope per element (edge_eval_ref.edge_stage_ref: layer
    1's add, four fmas and scale fma, the order-independent (64 + 2) u bound of layer 2 with layer 1's error through |W2|,
    the epilogue fma, the run sum, the reciprocal and the product, one rounding onto root; X6: + the three dropped cross
    terms); (b) TILES, every several-tiles form and WS_F32 return the same bits, as edge.hip claims; (c) a node without
    in-edges keeps its root row bit for bit; (d) so do the closed columns (t2 = -50) of every node; (e) below E = 64 the
    wave-specialised variants refuse and leave f_out as it was."""
    N, E, g, s, d, attr, row_ptr = _graph(name)
    inp, uvbuf = _fp32_operands(name, N, E, fold, 132 if name == "ladder" else 128)
    uvsnap = uvbuf.clone()
    refs = {x6: er.edge_stage_ref(inp, s, d, attr, N, x6=x6) for x6 in (False, True)}
    tag = "%s/%s" % (name, "fold" if fold else "unf")
    tiles = _run_fp32(inp, g, N, ("v", TILES))
    outs = {"TILES": tiles}
    for T in (2, 3, 16):
        outs["MT%d" % T] = _run_fp32(inp, g, N, ("mt", T))
    if E >= 64:
        outs["WS_F32"] = _run_fp32(inp, g, N, ("v", WS_F32))
        outs["WS_X6"] = _run_fp32(inp, g, N, ("v", WS_X6))
    else:
        fo, fbuf = _slot(N, 128, 64, 128)
        fo.copy_(inp["root"])
        snap = fbuf.clone()
        for v in (WS_F32, WS_X6):
            with pytest.raises(RuntimeError):
                _ops().edge_uv_mlp2_mean_eval(inp["UV"], g, inp["wc4"], inp["b1"],
                                              (inp["s1"], inp["t1"]) if inp["s1"] is not None else None, inp["W2"],
                                              inp["b2"], (inp["s2"], inp["t2"]), fo, variant=v)
            torch.cuda.synchronize()
            assert torch.equal(_bits(fbuf), _bits(snap))
    assert torch.equal(_bits(uvbuf), _bits(uvsnap))
    empty = torch.from_numpy(np.diff(row_ptr) == 0).to(DEV)
    cl = list(er.CLOSED)
    for route, got in outs.items():
        ref = refs[route == "WS_X6"]
        _worst(route, tag, got, ref["out"], ref["tol"])                                    # (a)
        if route not in ("TILES", "WS_X6"):
            assert torch.equal(_bits(got), _bits(tiles)), route                            # (b)
        assert torch.equal(_bits(got[empty]), _bits(inp["root"][empty])), route            # (c)
        assert torch.equal(_bits(got[:, cl]), _bits(inp["root"][:, cl])), route            # (d)
    tl = er.tile_layout(N, E)
    if tl["NG"] == 1:
        assert any(tl["tiles"] % T for T in (2, 3, 16))                 # some several-tiles form has a short last workgroup


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", ["ladder", "hub150", "u50_63", "u50_64", "u50_65"])
def test_edge_messages_fp32_match_fp64_per_element(name, fold):
    """yolat_edge_uv_mlp2_eval (k_edge_uv_mlp2: the messages H2 [E,64] of the two-kernel path) against the reference
    messages within their per-element bound, at E = 820, 2000 and around one 64-row tile; rows >= E and the columns
    beside the slot keep their NaN."""
    lib, check = _lib()
    N, E, g, s, d, attr, row_ptr = _graph(name)
    inp, _ = _fp32_operands(name, N, E, fold, 132 if name == "ladder" else 128)
    ref = er.edge_stage_ref(inp, s, d, attr, N)
    h2, hbuf = _slot(E, 72, 0, 64)

    def ptr(t):
        return None if t is None else t.data_ptr()

    def run():
        h2.fill_(NAN)
        snap = hbuf.clone()
        check(lib.yolat_edge_uv_mlp2_eval(inp["UV"].data_ptr(), inp["UV"].stride(0), g.src.data_ptr(), g.dst.data_ptr(),
                                          g.attr.data_ptr(), E, inp["wc4"].data_ptr(), ptr(inp["b1"]), ptr(inp["s1"]),
                                          ptr(inp["t1"]), inp["W2"].data_ptr(), ptr(inp["b2"]), ptr(inp["s2"]),
                                          ptr(inp["t2"]), 64, h2.data_ptr(), 72, _stream()), "yolat_edge_uv_mlp2_eval")
        assert _outside_untouched(hbuf, snap, E, 0, 64)
        return h2.clone()
    got = _twice(run)
    _worst("messages", "%s/%s" % (name, "fold" if fold else "unf"), got, ref["m"], ref["tol_m"])
    assert bool((got[:, list(er.CLOSED)] == 0).all())


@pytest.mark.parametrize("E", [131071, 131072])
def test_edge_stage_fp32_auto_route_flips_at_131072_edges(E):
    """The automatic choice (variant 0) on uniform(16000, E): node tiles below E = 131072 — the bits of TILES — and the
    wave-specialised X6 kernel from there on — the bits of WS_X6, which differ from those of TILES in at least one
    element (otherwise the comparison would say nothing about the route).  Both inside their envelopes.  Under
    YOLAT_STRICT_FP32=1 the large route is WS_F32, whose bits are those of TILES; WS_X6 must still differ."""
    N = 16000
    src, dst = er.br.uniform(N, E, seed=E)
    attr = er.randn32((E, 4), N + E + 1, 0.5)
    g, s, d, a, row_ptr = _build(N, src, dst, attr)
    inp = _dev(er.fold_inputs(er.stage_inputs(N, E, N + E)))
    auto = _run_fp32(inp, g, N, ("v", 0))
    tiles = _run_fp32(inp, g, N, ("v", TILES))
    x6 = _run_fp32(inp, g, N, ("v", WS_X6))
    assert not torch.equal(_bits(x6), _bits(tiles))
    strict = os.environ.get("YOLAT_STRICT_FP32", "")[:1] == "1"
    big = E >= 131072 and not strict
    assert torch.equal(_bits(auto), _bits(x6 if big else tiles))
    assert torch.equal(_bits(auto), _bits(tiles)) != big
    ref = er.edge_stage_ref(inp, s, d, a, N, x6=big)
    _worst("AUTO", "E=%d" % E, auto, ref["out"], ref["tol"])
    ref = er.edge_stage_ref(inp, s, d, a, N, x6=not big)
    _worst("WS_X6" if not big else "TILES", "E=%d" % E, tiles if big else x6, ref["out"], ref["tol"])


# ---------------------------------------------------------------------------------------------
# bf16 stage
# ---------------------------------------------------------------------------------------------
def _bf16_operands(N, E, ld_uv=128):
    inp = _dev(er.stage_inputs_bf16(N, E, N + E))
    uv, uvbuf = _slot(N, ld_uv, 0, 128, torch.bfloat16)
    uv.copy_(inp["UV"])
    inp["UV"] = uv
    root, _ = _slot(N, 72, 0, 64)
    root.copy_(inp["root"])
    inp["root"] = root
    return inp, uvbuf


def _call_bf16(inp, g, N, E, fo, variant):
    lib, _ = _lib()
    return lib.yolat_edge_uv_mlp2_mean_eval_bf16(inp["UV"].data_ptr(), inp["UV"].stride(0), g.src.data_ptr(), g.dst.data_ptr(),
                                                 g.attr.data_ptr(), g.row_ptr.data_ptr(), N, E, inp["wc4"].data_ptr(),
                                                 inp["s1"].data_ptr(), inp["W2f"].data_ptr(), inp["t2f"].data_ptr(),
                                                 inp["root"].data_ptr(), inp["root"].stride(0), fo.data_ptr(), 128, variant,
                                                 _stream())


def _run_bf16(inp, g, N, E, variant):
    """f_out [N,64] bf16 (columns 64:128 of a NaN-filled [N + 3, 128]), twice, the same bits, nothing outside touched"""
    _, check = _lib()
    fo, fbuf = _slot(N, 128, 64, 128, torch.bfloat16)

    def run():
        fo.fill_(NAN)
        snap = fbuf.clone()
        check(_call_bf16(inp, g, N, E, fo, variant), "yolat_edge_uv_mlp2_mean_eval_bf16")
        assert _outside_untouched(fbuf, snap, N, 64, 128)
        return fo.clone()
    return _twice(run)


def _check_bf16(tag, route, got, ref, inp, row_ptr):
    assert not bool(torch.isnan(got.float()).any()), "%s %s: a node was not written" % (route, tag)
    _worst(route, tag, got, ref["out"], ref["tol"])
    # how much of the bound is the flip allowance: the outputs that leave the base term (store half spacing + fp32 noise)
    err = (got.double() - ref["out"]).abs()
    print("beyond base %-20s %-16s %d of %d, worst error / base %.3f" % (
        route, tag, int((err > ref["base"]).sum()), err.numel(), float((err / ref["base"]).max())))
    empty =torch.from_numpy(np.diff(row_ptr) == 0).to(DEV)
    assert torch.equal(_bits(got[empty]), _bits(inp["root"][empty].to(torch.bfloat16))), route
    cl = list(er.CLOSED)
    assert torch.equal(_bits(got[:, cl]), _bits(inp["root"][:, cl].to(torch.bfloat16))), route


@pytest.mark.parametrize("name", er.BF16_GRAPHS)
def test_edge_stage_bf16_both_kernels_match_fp64_per_element(name):
    """yolat_edge_uv_mlp2_mean_eval_bf16, variant 1 (node tiles) and 2 (register-chained MFMA waves), on every table
    graph.  EVERY output inside the derived bound (edge_eval_ref.edge_stage_ref_bf16: the store's half spacing, the fp32
    noise, and one bf16 spacing of h1 through |W2f| for exactly those hidden activations whose float64 pre-activation lies
    within the kernel's layer-1 noise of a rounding midpoint) — no share is exempt; every node is written; a node without
    in-edges, and every closed column, holds the bf16 rounding of the root.  Below E = 16 the chained kernel refuses."""
    N, E, g, s, d, attr, row_ptr = _graph(name)
    inp, uvbuf = _bf16_operands(N, E, 136 if name == "ladder" else 128)
    uvsnap = uvbuf.clone()
    for variant, route, chain in ((1, "bf16 tiles", False), (2, "bf16 chained", True)):
        if chain and E < 16:
            fo, fbuf = _slot(N, 128, 64, 128, torch.bfloat16)
            snap = fbuf.clone()
            assert _call_bf16(inp, g, N, E, fo, 2) != 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(fbuf), _bits(snap))
            continue
        ref = er.edge_stage_ref_bf16(inp, s, d, attr, N, chain)
        print("flagged %-18s %-16s %.4f" % (route, name, ref["flagged"]))
        _check_bf16(name, route, _run_bf16(inp, g, N, E, variant), ref, inp, row_ptr)
    assert torch.equal(_bits(uvbuf), _bits(uvsnap))


@pytest.mark.parametrize("E", [15, 16])
def test_edge_chain_bf16_needs_sixteen_edges(E):
    """variant 2 on uniform(50, E): E = 15 returns YOLAT_E_UNSUPPORTED and writes nothing, E = 16 — one step of one stream
    — runs and is inside the bound"""
    lib, _ = _lib()
    N = 50
    src, dst = er.br.uniform(N, E, seed=E)
    attr = er.randn32((E, 4), N + E + 1, 0.5)
    g, s, d, a, row_ptr = _build(N, src, dst, attr)
    inp, _ = _bf16_operands(N, E)
    if E < 16:
        fo, fbuf = _slot(N, 128, 64, 128, torch.bfloat16)
        snap = fbuf.clone()
        rc = _call_bf16(inp, g, N, E, fo, 2)
        assert rc != 0 and b"support" in lib.yolat_strerror(int(rc)).lower()
        torch.cuda.synchronize()
        assert torch.equal(_bits(fbuf), _bits(snap))
        return
    ref = er.edge_stage_ref_bf16(inp, s, d, a, N, True)
    _check_bf16("E=16", "bf16 chained", _run_bf16(inp, g, N, E, 2), ref, inp, row_ptr)


@pytest.mark.parametrize("case", ["dense", "sparse"])
def test_edge_stage_bf16_automatic_choice(case):
    """variant 0: the chained kernel on hub(12000, 196609, 1000) (E >= 131072 and E >= 2 N) — the bits of variant 2; the
    node tiles on uniform(100000, 131072) (E < 2 N) — the bits of variant 1"""
    if case == "dense":
        N, E, g, s, d, attr, row_ptr = _graph("hub12000_196609")
        other = 2
    else:
        N, E = 100000, 131072
        src, dst = er.br.uniform(N, E, seed=E)
        g, s, d, attr, row_ptr = _build(N, src, dst, er.randn32((E, 4), N + E + 1, 0.5))
        other = 1
    inp, _ = _bf16_operands(N, E)
    auto, forced = _run_bf16(inp, g, N, E, 0), _run_bf16(inp, g, N, E, other)
    assert torch.equal(_bits(auto), _bits(forced))
    assert not torch.equal(_bits(auto), _bits(_run_bf16(inp, g, N, E, 3 - other)))     # the two kernels are told apart
