"""GPU tests (-m gpu) of the next layer's node side inside the eval edge launch (csrc/edge.hip, EdgeNext of internal.hpp):
k_edge_uv_mlp2_mean<1, true> fetches the packed weight's B fragments in one batch, and k_edge_mt_uv_mlp2_mean<true> runs the
node side once per workgroup, after its last tile, on rows re-read from f_out and staged four tiles at a time.

Through yolat_debug_edge_uv_mlp2_mean_eval_next (the edge op with an EdgeNext, as the eval forward's chain launches it):
  * N = 45 with one hub of 70 in-edges (two 64-edge passes) and one node without in-edges, in tiles of 10 nodes (E = 250:
    five tiles, the last of 5 nodes; at T = 2 the last workgroup owns one tile, at T = 5 the one workgroup stages 4 + 1)
    and in tiles of 4 nodes (E = 600: twelve tiles, the last of 1 node; at T = 5 the groups are 4 + 1, 4 + 1, 2); both
    fold settings; f_out, UV', root' and s' at T = 2, 3, 4, 5 must hold the BYTES of T = 1;
  * N = 11 in one tile (nn = 11 < 16): the row masking; rows the launch does not own keep their NaN fill;
  * T = 1 against float64.  tests/test_gpu_fp32_graph_ops.py has no figure for this fused op: the envelope here is composed
    per element from the pieces tests/graph_ref.py gives for its parts (u = 2^-24):
      h1   edge_uv_lin1_ref's 6 u S, + u |t1| for the folded BatchNorm's one fma (ReLU is continuous: no term);
      msg  dot_delta(|h1| . |W2| + |b2|, 64) + |W2| . d(h1), then u |t2| + |s2| d for the fma;
      f    csr_mean_fwd_ref's mean and accumulate envelopes on the messages + the mean of d(msg);
      UV' | root'   dot_delta(|f| . |W'| + |bias|, 64) + |W'| . d(f);      s'   dot_delta(|s| . |Wn| + |bn|, 64), u |t| for the fma.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr
from bf16_ref import dot_delta

pytestmark = pytest.mark.gpu
U = gr.U
HUB, LONE = 7, 23
TS = (2, 3, 4, 5)


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _fn():
    lib = _yv()._lib.lib
    fn = lib.yolat_debug_edge_uv_mlp2_mean_eval_next
    p, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn.restype = ci
    fn.argtypes = ([p, i64, p, p, p, p, i64, i64] + [p] * 8 + [i64, p, i64, ci] + [p, p, p, i64, p, i64, p, i64] + [p] * 4 +
                   [p, i64, ctypes.POINTER(ci), p])
    return fn


def _edges(N, E, hub_deg, seed):
    """(src, dst) int64: node HUB has exactly hub_deg in-edges, node LONE none, the rest uniform (N > 16); N <= 16: uniform
    over all nodes but the last, which has no in-edge"""
    rng = np.random.default_rng(seed)
    if N <= 16:
        return rng.integers(0, N, E), rng.integers(0, N - 1, E)
    pool = np.array([n for n in range(N) if n not in (HUB, LONE)])
    dst = np.concatenate([np.full(hub_deg, HUB), pool[rng.integers(0, len(pool), E - hub_deg)]])
    return rng.integers(0, N, E), dst[rng.permutation(E)]


def _pack_wp(W):
    """Wp[(ct * 16 + ks) * 64 + l] = W'[ct * 16 + (l & 15)][4 * ks + (l >> 4)]   (internal.hpp)"""
    return W.reshape(12, 16, 16, 4).permute(0, 2, 3, 1).contiguous().reshape(-1)


_CASES = {}


def _case(N, E, fold):
    """inputs, the graph, the outputs at every T and the float64 reference with its envelope: computed once, read by all"""
    key = (N, E, fold)
    if key in _CASES:
        return _CASES[key]
    yv = _yv()
    src, dst = _edges(N, E, 70, 1000 * N + E)
    tg = torch.Generator().manual_seed(7 * N + E)
    rn = lambda *s: torch.randn(*s, generator=tg)
    attr = rn(E, 4)
    g = yv.ops.build_graph(torch.from_numpy(np.stack([src, dst], 1).astype(np.int64)).cuda(), attr.cuda(), None, N, 1)
    g.check_status()
    ps = lambda: (torch.rand(64, generator=tg) + 0.5, rn(64) * 0.2)
    c = dict(UV=rn(N, 128), wc4=rn(64, 4) / 2, W2=rn(64, 64) / 8, p2=ps(), root=rn(N, 64), Wx=rn(192, 64) / 8, bx=rn(192) * 0.1,
             s_in=rn(N, 64), Wn=rn(64, 64) / 8, bn=rn(64) * 0.1, pn=ps())
    c["b1"], c["p1"], c["b2"] = (None, None, None) if fold else (rn(64) * 0.1, ps(), rn(64) * 0.1)
    d = {k: (tuple(t.cuda() for t in v) if isinstance(v, tuple) else (v.cuda() if v is not None else None)) for k, v in c.items()}
    wp = _pack_wp(d["Wx"])
    ptr = lambda t: t.data_ptr() if t is not None else None
    s1, t1 = d["p1"] if d["p1"] is not None else (None, None)
    fn = _fn()

    def run(T):
        f = torch.full((N, 128), float("nan"), device="cuda")       # f_out in a column slot, as in the forward
        f[:, 64:] = d["root"]
        uvn = torch.full((N, 132), float("nan"), device="cuda")
        rt = torch.full((N, 68), float("nan"), device="cuda")
        so = torch.full((N, 68), float("nan"), device="cuda")
        fo = f[:, 64:]
        did = ctypes.c_int(0)
        rc = fn(ptr(d["UV"]), 128, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(), g.row_ptr.data_ptr(), N, E,
                ptr(d["wc4"]), ptr(d["b1"]), ptr(s1), ptr(t1), ptr(d["W2"]), ptr(d["b2"]), ptr(d["p2"][0]), ptr(d["p2"][1]),
                64, fo.data_ptr(), 128, T, ptr(wp), ptr(d["bx"]), uvn.data_ptr(), 132, rt.data_ptr(), 68, ptr(d["s_in"]), 64,
                ptr(d["Wn"]), ptr(d["bn"]), ptr(d["pn"][0]), ptr(d["pn"][1]), so.data_ptr(), 68, ctypes.byref(did),
                yv.ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and did.value == 1, (rc, did.value)
        return dict(f=f, uvn=uvn, root=rt, s=so)

    npt = max(1, min(64, 56 * N // E))
    outs = {T: run(T) for T in (1,) + TS}
    _CASES[key] = (d, g, outs, npt)
    return _CASES[key]


SHAPES = [(45, 250), (45, 600), (11, 40)]


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("N,E", SHAPES)
def test_next_node_side_is_bit_identical_at_every_tiles_per_workgroup(N, E, fold):
    d, g, outs, npt = _case(N, E, fold)
    deg = torch.bincount(g.dst[:E].long(), minlength=N)
    tiles = -(-N // npt)
    if N == 45:
        assert int(deg[HUB]) == 70 and int(deg[LONE]) == 0
        assert (npt, tiles, N - (tiles - 1) * npt) in ((10, 5, 5), (4, 12, 1))
    else:
        assert tiles == 1 and N < 16 and int(deg[N - 1]) == 0
    want = outs[1]
    # the launch wrote every row it owns and nothing else: the padding columns keep their fill
    assert torch.isfinite(want["f"][:, 64:]).all() and torch.isnan(want["f"][:, :64]).all()
    assert torch.isfinite(want["uvn"][:, :128]).all() and torch.isnan(want["uvn"][:, 128:]).all()
    for k in ("root", "s"):
        assert torch.isfinite(want[k][:, :64]).all() and torch.isnan(want[k][:, 64:]).all()
    assert torch.equal(want["f"][deg == 0, 64:], d["root"][deg == 0])          # no in-edge: the root term as it came
    for T in TS:
        for k, a in want.items():
            b = outs[T][k]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (N, E, fold, T, k)


def _envelope(d, g, N, E):
    """float64 reference and per-element tolerance of (f_out, UV' | root', s'): the docstring's composition"""
    dst, src, attr = g.dst[:E].long(), g.src[:E].long(), g.attr[:E]
    h, dh = gr.edge_uv_lin1_ref(d["UV"], src, dst, attr, d["wc4"], d["b1"])
    if d["p1"] is not None:
        s1, t1 = d["p1"][0].double(), d["p1"][1].double()
        t = h * s1 + t1
        dh = dh * s1.abs() + U * t.abs()
        h = t
    h1 = torch.relu(h)
    W2 = d["W2"].double()
    b2 = d["b2"].double() if d["b2"] is not None else torch.zeros(64, dtype=torch.float64, device="cuda")
    z = h1 @ W2.t() + b2
    dz = dot_delta(h1.abs() @ W2.abs().t() + b2.abs(), 64) + dh @ W2.abs().t()
    s2, t2 = d["p2"][0].double(), d["p2"][1].double()
    t = z * s2 + t2
    dm = dz * s2.abs() + U * t.abs()
    msg = torch.relu(t)
    f, tol_f, deg = gr.csr_mean_fwd_ref(msg, None, None, False, dst, N, base=d["root"])
    d1 = deg.clamp_min(1)[:, None]
    tol_f = (tol_f + torch.zeros(N, 64, dtype=torch.float64, device="cuda").index_add_(0, dst, dm) / d1) * gr.SLACK
    Wx, bx = d["Wx"].double(), d["bx"].double()
    nx = f @ Wx.t() + bx
    tol_nx = (dot_delta(f.abs() @ Wx.abs().t() + bx.abs(), 64) + tol_f @ Wx.abs().t()) * gr.SLACK
    s, Wn, bn = d["s_in"].double(), d["Wn"].double(), d["bn"].double()
    sn, tn = d["pn"][0].double(), d["pn"][1].double()
    zs = s @ Wn.t() + bn
    ts = zs * sn + tn
    tol_s = (dot_delta(s.abs() @ Wn.abs().t() + bn.abs(), 64) * sn.abs() + U * ts.abs()) * gr.SLACK
    return (f, tol_f), (nx, tol_nx), (torch.relu(ts), tol_s)


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("N,E", SHAPES)
def test_one_tile_per_workgroup_matches_fp64(N, E, fold):
    d, g, outs, npt = _case(N, E, fold)
    got = outs[1]
    (f, tol_f), (nx, tol_nx), (s, tol_s) = _envelope(d, g, N, E)
    pairs = (("f_out", got["f"][:, 64:], f, tol_f), ("UV'", got["uvn"][:, :128], nx[:, :128], tol_nx[:, :128]),
             ("root'", got["root"][:, :64], nx[:, 128:], tol_nx[:, 128:]), ("s'", got["s"][:, :64], s, tol_s))
    worst = {}
    for name, a, want, tol in pairs:
        assert float(tol.min()) > 0.0
        worst[name] = float(((a.double() - want).abs() / tol).max())
    print("N=%d E=%d fold=%s: worst error / tolerance %s" % (N, E, fold, ", ".join("%s %.3f" % kv for kv in worst.items())))
    for name, w in worst.items():
        assert w <= 1.0, (name, w)
