"""GPU tests (-m gpu) of the eval forward's throughput regime (csrc/forward_eval.hip yolat_eval_regime_*): the shapes it
selects — k_prep_small with 250-row workgroups and the several-tiles-per-workgroup edge kernel
(csrc/edge.hip k_edge_mt_uv_mlp2_mean) — must give the SAME BYTES as the one-forward-at-a-time launches.

(a) the edge op alone through yolat_edge_uv_mlp2_mean_eval_mt, tiles_per_wg 2 / 3 / 4 against 1;
(b) the whole forward with the regime forced to throughput against forced latency (the chain instance that carries the next
    layer's node side, and the pooling rider);
(c) eight streams with four forwards each in auto mode against the one-stream result.
Bit equality needs no tolerance: per tile the new kernel runs the one-tile kernel's products, sums and roundings in its
order, and k_prep_small builds the same arrays at every rows-per-workgroup."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu

pytestmark = pytest.mark.gpu


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _graphs():
    """name -> (src, dst, N): seeded"""
    rng = np.random.default_rng(41)
    out = {}
    # 8 tiles of 14 nodes: at 3 tiles per workgroup the last workgroup is short
    out["uniform_100"] = (rng.integers(0, 100, 400), rng.integers(0, 100, 400), 100)
    # fewer tiles than a workgroup of 4 can own
    out["tiny_15"] = (rng.integers(0, 15, 60), rng.integers(0, 15, 60), 15)
    # tiles of 7 nodes: node 3 holds 200 edges (four 64-edge passes in tile 0), nodes 7..14 none (tile 1 is empty),
    # the other 312 edges go to the rest
    rest = np.array([n for n in range(64) if n != 3 and not 7 <= n <= 14])
    dst = np.concatenate([np.full(200, 3), rest[rng.integers(0, len(rest), 312)]])
    out["hub_and_empty_64"] = (rng.integers(0, 64, 512), dst[rng.permutation(512)], 64)
    out["ragged_1009"] = (rng.integers(0, 1009, 4001), rng.integers(0, 1009, 4001), 1009)
    return out


GRAPHS = _graphs()


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_edge_tiles_per_workgroup_are_bit_identical(name, fold):
    yv = _yv()
    src, dst, N = GRAPHS[name]
    E = len(src)
    deg = np.bincount(dst, minlength=N)
    if name == "hub_and_empty_64":
        assert deg[3] == 200 and (deg[7:15] == 0).all() and 56 * N // E == 7
    tg = torch.Generator().manual_seed(N + E)
    attr = torch.randn(E, 4, generator=tg)
    g = yv.ops.build_graph(torch.from_numpy(np.stack([src, dst], 1).astype(np.int64)).cuda(), attr.cuda(), None, N, 1)
    g.check_status()
    UV = torch.randn(N, 128, generator=tg).cuda()
    wc4 = (torch.randn(64, 4, generator=tg) / 2).cuda()
    W2 = (torch.randn(64, 64, generator=tg) / 8).cuda()
    vec = lambda s: (torch.randn(64, generator=tg) * s).cuda()
    p2 = ((torch.rand(64, generator=tg) + 0.5).cuda(), vec(0.2))
    b1, p1, b2 = (None, None, None) if fold else (vec(0.1), ((torch.rand(64, generator=tg) + 0.5).cuda(), vec(0.2)), vec(0.1))
    root = torch.randn(N, 128, generator=tg).cuda()               # f_out arrives holding the root term, in a column slot

    def run(T):
        f = root.clone()
        yv.ops.edge_uv_mlp2_mean_eval_mt(UV, g, wc4, b1, p1, W2, b2, p2, f[:, 64:], tiles_per_wg=T)
        torch.cuda.synchronize()
        return f

    want = run(1)
    plain = root.clone()
    yv.ops.edge_uv_mlp2_mean_eval(UV, g, wc4, b1, p1, W2, b2, p2, plain[:, 64:], variant=yv.ops.EDGE_TILES)
    assert torch.equal(want, plain)                               # tiles_per_wg = 1 is the one-tile kernel
    assert torch.equal(want[:, :64], root[:, :64]) and not torch.equal(want[:, 64:], root[:, 64:])
    for T in (2, 3, 4):
        got = run(T)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, T, float((got - want).abs().max()))
    for bad in (0, 17):
        with pytest.raises(RuntimeError):
            run(bad)


def _to_device(data):
    for k in ("x", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
        data[k] = data[k].cuda()
    return data


def _tensors(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [t for t in out if torch.is_tensor(t)]


def _forward(model, data, slices):
    data._yolat_stage = None                                      # rebuild the CSR: k_prep_small is part of the regime
    with torch.no_grad():
        return [t.clone() for t in _tensors(model(data, slices))]


def _cases():
    yv = _yv()
    small, sl = yv.synth_batch(1, 77, num_proposals=12, nodes_lo=25, nodes_hi=25, edges_per_proposal=100)
    d2, s2, kw2, _ = yv.config("2")
    return [("small", small, sl, dict(n_classes=17, n_blocks=2, n_blocks_out=2)), ("cfg2", d2, s2, kw2)]


def test_whole_forward_is_bit_identical_in_both_regimes():
    yv = _yv()
    lib = yv._lib.lib
    try:
        for name, data, slices, optkw in _cases():
            model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 5).cuda().eval()
            _to_device(data)
            counts0 = (ctypes.c_int64 * 2)()
            lib.yolat_eval_regime_counts(counts0)
            assert lib.yolat_eval_regime_set(1) == 0
            want = _forward(model, data, slices)
            assert lib.yolat_eval_regime_set(2) == 0
            got = _forward(model, data, slices)
            torch.cuda.synchronize()
            counts1 = (ctypes.c_int64 * 2)()
            lib.yolat_eval_regime_counts(counts1)
            assert counts1[0] - counts0[0] == 1 and counts1[1] - counts0[1] == 1, (list(counts0), list(counts1))
            assert len(want) == len(got) >= 1
            for a, b in zip(want, got):
                assert a.shape == b.shape and a.dtype == b.dtype
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, float((a.float() - b.float()).abs().max()))
            assert torch.isfinite(want[0]).all() and float(want[0].abs().max()) > 0
    finally:
        lib.yolat_eval_regime_set(0)


def test_eight_streams_in_auto_mode_match_the_one_stream_result():
    yv = _yv()
    lib = yv._lib.lib
    try:
        lib.yolat_eval_regime_set(0)
        name, data, slices, optkw = _cases()[0]
        model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 6).cuda().eval()
        _to_device(data)
        lib.yolat_eval_regime_set(1)
        want = _forward(model, data, slices)
        torch.cuda.synchronize()
        lib.yolat_eval_regime_set(0)
        counts0 = (ctypes.c_int64 * 2)()
        lib.yolat_eval_regime_counts(counts0)
        streams = [torch.cuda.Stream() for _ in range(8)]
        outs = []
        for rep in range(4):
            for st in streams:
                with torch.cuda.stream(st):
                    outs.append(_forward(model, data, slices))
        torch.cuda.synchronize()
        counts1 = (ctypes.c_int64 * 2)()
        lib.yolat_eval_regime_counts(counts1)
        print("forwards per regime (latency, throughput):", counts1[0] - counts0[0], counts1[1] - counts0[1])
        assert (counts1[0] - counts0[0]) + (counts1[1] - counts0[1]) == 32
        for got in outs:
            for a, b in zip(want, got):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    finally:
        lib.yolat_eval_regime_set(0)
