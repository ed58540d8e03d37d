"""float64 reference, error envelope, exact probes, layouts and a CPU emulation of the one-launch proposal-local conv stack
of the bf16-storage eval forward (csrc/conv_local.hip, k_conv_local_h<NW, COO>).  CPU only: torch and numpy, no import of
the extension.  tests/test_conv_local_ref_host.py checks every claim made here; tests/test_gpu_conv_local_elements.py
holds the kernel to it.

The arithmetic of one layer (header of conv_local.hip), with the folded operands the eval plan builds:
    node phase   U' | V' | R | S = W' . in + shift,  W' = [Wuv * uv_scale ; Wr ; Wn * sn]  (U', V', R from the f rows, S from s)
                 s = relu(S)
    edge phase   h1 = relu(U'[dst] + V'[src] + Wc4f . attr),  Wc4f = Wc4 * s1
                 m  = relu(W2f . h1 + t2f)
                 f  = R + sum_in-edges m / max(deg, 1)
    pooled       Z_max = max of the stored f rows per proposal,  Z_mean = sum s / max(cnt, 1)
The kernel stores U', V', s, h1, m (on entry to the aggregation MFMA) and f as bfloat16 (round to nearest even) and
accumulates in fp32; R stays fp32.  A reference value is computed in float64 with no intermediate rounding, FROM THE ROWS
THE KERNEL STORED for the previous layer, and comes with a per-element envelope built from that element's own operand
magnitudes (layer_want).  Nothing here is scaled by a tensor maximum or an rms.
"""
import numpy as np
import torch

import bf16_ref as br

C = 64
EPS32 = br.EPS32

# (hi, lo) operand pairs, three of the four cross terms (layer 0's node phase: x and W; every edge phase: e_attr and Wc4f).
# For fp32 v in [2^e, 2^(e+1)): hi = bf16(v), r = v - hi (exact in fp32), |r| <= 2^(e-8) (half a bf16 spacing).  Either
# |r| = 2^(e-8), a power of two and its own bf16, or floor(log2 |r|) <= e - 9 and lo = bf16(r) is within half a spacing
# there, 2^(e-17) <= 2^-17 |v|.  So hi + lo = v (1 + d), |d| <= 2^-17, and |lo| <= 2^-8 |v| (1 + 2^-8).
#   (w_hi + w_lo)(x_hi + x_lo) - w_lo x_lo = w x (1 + d_w)(1 + d_x) - w_lo x_lo
#   |error| <= |w||x| (2^-17 + 2^-17 + 2^-34 + 2^-16 (1 + 2^-8)^2) <= 2^-15 (1 + 2^-8) |w||x|
SPLIT3 = 2.0 ** -15 * (1.0 + 2.0 ** -8)


def half_ulp(v):
    return 0.5 * br.ulp_bf16(v)


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
def model_convs(model):
    net = model.cls_net
    return [net.head.gconv] + [blk.body.gconv for blk in net.backbone]


def _bn_fold(bn, dtype):
    """eval BatchNorm as (scale, shift): invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale
    (k_bn_eval_coeffs), every step rounded to `dtype`"""
    eps = torch.tensor(bn.eps, dtype=torch.float32).to(dtype)
    invstd = 1.0 / torch.sqrt(bn.running_var.detach().to(dtype) + eps)
    sc = bn.weight.detach().to(dtype) * invstd
    return sc, bn.bias.detach().to(dtype) - bn.running_mean.detach().to(dtype) * sc


def fold_state(model, dtype=torch.float32):
    """The folded operands of every conv layer the way EvalPlan builds them (plan.py: _build_conv, _build_bf16), on the
    CPU: a list of dicts  Wuv [128,Cin], uv_scale, uv_shift [128], Wc4 [64,4], s1 [64], Wr [64,Cin], br, Wn [64,Cin], bn,
    sn, tn [64], W2f [64,64] (bfloat16 when dtype is fp32: the plan's half_folded), t2f [64].  dtype float64: the same
    formulas without rounding (W2f stays float64) — the operands of the unrounded want."""
    out = []
    for cv in model_convs(model):
        cin = cv.in_channels
        W1 = cv.nn[0].weight.detach().to(dtype)
        s1, t1 = _bn_fold(cv.nn[1], dtype)
        s2, t2 = _bn_fold(cv.nn[4], dtype)
        sn, tn = _bn_fold(cv.mlp_node[1], dtype)
        w1a, w1b = W1[:, :cin], W1[:, cin:2 * cin]
        W2f = cv.nn[3].weight.detach().to(dtype) * s2[:, None]
        out.append(dict(
            Cin=cin, Wuv=torch.cat([w1a - w1b, w1b], 0).contiguous(), Wc4=W1[:, 2 * cin:].contiguous(),
            uv_scale=torch.cat([s1, s1]), uv_shift=torch.cat([s1 * cv.nn[0].bias.detach().to(dtype) + t1, torch.zeros_like(t1)]),
            s1=s1, Wr=cv.lin_r.weight.detach().to(dtype), br=cv.lin_r.bias.detach().to(dtype),
            Wn=cv.mlp_node[0].weight.detach().to(dtype), bn=cv.mlp_node[0].bias.detach().to(dtype), sn=sn, tn=tn,
            W2f=W2f.to(torch.bfloat16) if dtype == torch.float32 else W2f,
            t2f=s2 * cv.nn[3].bias.detach().to(dtype) + t2))
    return out


def pack_layer(op, layer, rounded=True):
    """What k_conv_local_pack makes of a layer's folded operands, as float64 tensors:
        W [256,Cin]  the stacked node weight U | V | root | node branch: ONE multiply in the operands' precision by the
                     BatchNorm scale, then — layers >= 1 — round to nearest even to bfloat16 (layer 0 keeps the fp32
                     product: it enters the kernel as a (hi, lo) pair)
        shift [256]  uv_shift | br | bn sn + tn;  shift_mag: the magnitudes |bn sn| + |tn| behind its last 64 entries
        Wc [64,4]    Wc4 * s1 (fp32 product; a (hi, lo) pair in the kernel),  W2f [64,64], t2f [64]
    rounded=False (float64 operands from fold_state): no rounding anywhere."""
    W = torch.cat([op["Wuv"] * op["uv_scale"][:, None], op["Wr"], op["Wn"] * op["sn"][:, None]], 0)
    if rounded and layer > 0:
        W = W.to(torch.bfloat16)
    bs = op["bn"].double() * op["sn"].double()
    shift = torch.cat([op["uv_shift"].double(), op["br"].double(), bs + op["tn"].double()])
    mag = torch.cat([op["uv_shift"].double().abs(), op["br"].double().abs(), bs.abs() + op["tn"].double().abs()])
    return dict(layer=layer, Cin=op["Cin"], W=W.double(), shift=shift, shift_mag=mag,
                Wc=(op["Wc4"] * op["s1"][:, None]).double(), W2f=op["W2f"].double(), t2f=op["t2f"].double())


def pack_model(ops, rounded=True):
    return [pack_layer(op, l, rounded) for l, op in enumerate(ops)]


# ---------------------------------------------------------------------------------------------
# graph structure
# ---------------------------------------------------------------------------------------------
class Csr(object):
    """The destination-sorted (stable) form of a layout's edge list, as the kernel sees it: src, dst, perm [E] int64,
    row_ptr [N+1], deg [N], seg_ptr [P+1], cnt [P]."""

    def __init__(self, edge, bbox_idx, N, P):
        edge = torch.as_tensor(edge, dtype=torch.int64)
        bb = torch.as_tensor(bbox_idx, dtype=torch.int64)
        self.N, self.P, self.E = int(N), int(P), int(edge.shape[0])
        self.perm = torch.argsort(edge[:, 1], stable=True)
        self.src, self.dst = edge[self.perm, 0], edge[self.perm, 1]
        self.deg = torch.bincount(self.dst, minlength=self.N)
        self.row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(self.deg, 0)])
        self.cnt = torch.bincount(bb, minlength=self.P)
        self.seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(self.cnt, 0)])
        self.bbox_idx = bb


def default_g0(P, NW):
    """proposals per workgroup the launcher picks (yl_conv_local_bf16)"""
    slots = 256 if NW == 8 else 512
    return int(min(max((P + slots - 1) // slots, 4), 64))


def tile_plan(g, NW, g0=0):
    """The kernel's greedy tiling and stream split, restated: (tiles, flag).  A workgroup owns g0 consecutive proposals
    and packs them, in order, into tiles of <= T = 16 NW nodes and <= ET = 128 NW edges; a proposal that fits no tile
    raises the flag and is skipped.  Per tile: n0, nt, e0, et (node / CSR-edge range), p0, p1 (proposals) and ns
    [2 NW + 1], the tile-local node boundaries of the 2 NW edge streams: edge-balanced, node-aligned, then clamped so
    that every stream holds <= 16 nodes and the rest still fits (`cand`: the boundaries before the clamp)."""
    T, ET, NS = 16 * NW, 128 * NW, 2 * NW
    g0 = int(g0) if g0 else default_g0(g.P, NW)
    seg, rp = g.seg_ptr.tolist(), g.row_ptr.tolist()
    dst = g.dst.tolist()
    tiles, flag = [], 0
    for w0 in range(0, g.P, g0):
        w1 = min(w0 + g0, g.P)
        q0 = w0
        while q0 < w1:
            q1 = q0
            while q1 < w1 and seg[q1 + 1] - seg[q0] <= T and rp[seg[q1 + 1]] - rp[seg[q0]] <= ET:
                q1 += 1
            if q1 == q0:
                flag = 1
                q0 += 1
                continue
            n0, nt, e0 = seg[q0], seg[q1] - seg[q0], rp[seg[q0]]
            et = rp[seg[q1]] - e0
            cand = []
            for k in range(NS + 1):
                if k >= NS:
                    cand.append(nt)
                elif et > 0:
                    tgt = (et * k) // NS
                    d = dst[e0 + min(tgt, et - 1)] - n0
                    cand.append(d if rp[n0 + d] - e0 == tgt else d + 1)
                else:
                    cand.append((nt * k) // NS)
            ns = [0]
            for k in range(1, NS + 1):
                lob, hib = max(ns[-1], nt - 16 * (NS - k)), min(ns[-1] + 16, nt)
                ns.append(min(max(cand[k], lob), hib))
            tiles.append(dict(n0=n0, nt=nt, e0=e0, et=et, p0=q0, p1=q1, ns=ns, cand=cand))
            q0 = q1
    return tiles, flag


# ---------------------------------------------------------------------------------------------
# float64 want + envelope, one layer at a time
# ---------------------------------------------------------------------------------------------
def _node_phase(pk, rows, vin, ein):
    """float64 (out, delta) of rows `rows` of the stacked node product on input vin [N,K] known to within ein (>= 0, same
    shape, or None): delta = |W'| ein + the fp32 accumulation bound of the product (dot_delta over the MFMA's K: 64, or
    the two 16-wide k-steps of layer 0) + layer 0's (hi, lo) term SPLIT3 |w||x| + two fp32 roundings of the shift."""
    W, sh = pk["W"][rows], pk["shift"][rows]
    out = vin @ W.t() + sh
    prod = vin.abs() @ W.abs().t()
    carried = ein @ W.abs().t() if ein is not None else torch.zeros_like(prod)
    K = 32 if pk["layer"] == 0 else 64
    delta = carried + br.dot_delta(prod + carried + sh.abs(), K) + 2.0 * EPS32 * pk["shift_mag"][rows]
    if pk["layer"] == 0:
        delta = delta + SPLIT3 * prod
    return out, delta


def layer_want(pk, fin, attr, g):
    """(want, tol, parts) of the f rows of one layer in float64.  fin [N,Cin]: the layer's input rows — x for layer 0,
    the rows the kernel stored for the previous layer otherwise (exact operands either way); attr [E,4] in CSR order.
    The envelope follows the kernel's storage points:
        U', V'   delta_node + 1/2 ulp_bf16                                   (R: delta_node only, it stays fp32)
        z        e_U[dst] + e_V[src] + SPLIT3 |Wc4f||attr| + dot_delta(., 16)  ->  h1: + 1/2 ulp_bf16 (ReLU is 1-Lipschitz)
        m        |W2f| e_h1 + dot_delta(., 64 + 3) + 1/2 ulp_bf16             (t2f enters as three exact bf16 terms)
        sum      sum e_m + dot_delta(sum (|m| + e_m), deg)
        f        e_sum / deg + e_R + 3 2^-24 (sum |m| / deg + |R|)   (1 / deg rounded, one fma), then the bf16 store:
                 store_envelope"""
    fin, attr = fin.double(), attr.double()
    out, d = _node_phase(pk, slice(0, 3 * C), fin, None)
    U, V, R = out[:, :C], out[:, C:2 * C], out[:, 2 * C:]
    eU = d[:, :C] + half_ulp(U.abs() + d[:, :C])
    eV = d[:, C:2 * C] + half_ulp(V.abs() + d[:, C:2 * C])
    eR = d[:, 2 * C:]
    dst, src = g.dst, g.src
    wa, wa_mag = attr @ pk["Wc"].t(), attr.abs() @ pk["Wc"].abs().t()
    z = U[dst] + V[src] + wa
    e_in = eU[dst] + eV[src]
    e_z = e_in + SPLIT3 * wa_mag + br.dot_delta(U[dst].abs() + V[src].abs() + wa_mag + e_in, 16)
    h1 = torch.relu(z)
    e_h1 = e_z + half_ulp(z.abs() + e_z)
    W2a = pk["W2f"].abs().t()
    mp = h1 @ pk["W2f"].t() + pk["t2f"]
    carried = e_h1 @ W2a
    e_mp = carried + br.dot_delta((h1 + e_h1) @ W2a + pk["t2f"].abs(), C + 3)
    m = torch.relu(mp)
    e_m = e_mp + half_ulp(mp.abs() + e_mp)
    N = fin.shape[0]
    zero = torch.zeros(N, C, dtype=torch.float64)
    agg = zero.index_add(0, dst, m)
    e_sum = zero.index_add(0, dst, e_m)
    deg = g.deg.double()[:, None]
    e_agg = e_sum + br.dot_delta(agg + e_sum, deg)
    dc = deg.clamp(min=1)
    want = R + agg / dc
    d_f = e_agg / dc + eR + 3.0 * EPS32 * (agg / dc + R.abs())
    return want, br.store_envelope(want, d_f), dict(U=U, V=V, R=R, h1=h1, m=m, agg=agg)


def s_chain(pks, x, g):
    """The node branch and its pooled mean, layer by layer in float64: a list of (Zmean [P,64], tol [P,64], s, err).  The s
    rows are not stored by the kernel, so their envelope travels: err_l <= |Wn'| err_(l-1) + delta + 1/2 ulp_bf16 (ReLU
    is 1-Lipschitz); the mean adds the fp32 accumulation over the proposal's rows and the rounded 1 / cnt."""
    out = []
    s, err = x.double(), None
    cnt = g.cnt.double()[:, None]
    cc = cnt.clamp(min=1)
    for pk in pks:
        pre, d = _node_phase(pk, slice(3 * C, 4 * C), s, err)
        s = torch.relu(pre)
        err = d + half_ulp(pre.abs() + d)
        zero = torch.zeros(g.P, C, dtype=torch.float64)
        tot, etot = zero.index_add(0, g.bbox_idx, s), zero.index_add(0, g.bbox_idx, err)
        zmean = tot / cc
        tol = (etot + br.dot_delta(tot + etot, cnt)) / cc + 3.0 * EPS32 * zmean
        out.append((zmean, tol, s, err))
    return out


def unrounded_forward(model, x, edge, e_attr, bbox_idx, P):
    """(f per layer, Zmean per layer) of the float64 want chained through its own layers on unrounded float64 operands:
    what oracle_torch.Backbone computes in float64 on the same state"""
    pks = pack_model(fold_state(model, torch.float64), rounded=False)
    g = Csr(edge, bbox_idx, x.shape[0], P)
    attr = torch.as_tensor(e_attr).double()[g.perm]
    fs, fin = [], torch.as_tensor(x).double()
    for pk in pks:
        fin = layer_want(pk, fin, attr, g)[0]
        fs.append(fin)
    return fs, [z[0] for z in s_chain(pks, torch.as_tensor(x), g)]


def check_feats(feats, x, attr_csr, pks, g):
    """The assertion of the GPU test on the stored f rows: feats [N, 64 L] bfloat16 (every layer's rows, n_blocks_out ==
    n_blocks).  Layer l is held to layer_want on the rows stored for layer l - 1.  Returns a list per layer of
    (worst |err| / tol, number of elements outside the envelope, index of the worst element, worst |err| / tol among
    the nodes WITH in-edges — a node without any is held to half a spacing of R, which rounding alone nearly fills)."""
    res = []
    f = feats.double()
    for l, pk in enumerate(pks):
        fin = x.double() if l == 0 else f[:, C * (l - 1):C * l]
        want, tol, _ = layer_want(pk, fin, attr_csr, g)
        got = f[:, C * l:C * (l + 1)]
        ratio = (got - want).abs() / tol
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
        worst = int(torch.argmax(ratio))
        fed = ratio[g.deg > 0]
        res.append((float(ratio.max()) if ratio.numel() else 0.0, int((ratio > 1.0).sum()), (worst // C, worst % C),
                    float(fed.max()) if fed.numel() else 0.0))
    return res


def check_zmean(zmean, x, pks, g):
    """The assertion on Z[:, 2F + D:] (the per-proposal mean of the node branch of every layer) against s_chain."""
    res = []
    for l, (want, tol, _, _) in enumerate(s_chain(pks, x, g)):
        got = zmean[:, C * l:C * (l + 1)].double()
        ratio = (got - want).abs() / tol.clamp(min=2.0 ** -133)
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
        res.append((float(ratio.max()), int((ratio > 1.0).sum())))
    return res


def pooled_max(feats, g):
    """Z[:, F:F + D] as the kernel defines it: the max of the stored rows of every proposal, 0 for one without nodes"""
    D = feats.shape[1]
    out = torch.full((g.P, D), -float("inf")).scatter_reduce(0, g.bbox_idx[:, None].expand(-1, D), feats.float(), "amax",
                                                            include_self=True)
    return torch.where((g.cnt > 0)[:, None], out, torch.zeros_like(out))


# ---------------------------------------------------------------------------------------------
# exact counting probes
# ---------------------------------------------------------------------------------------------
def unit_running_var(eps=1e-5):
    """a float32 running_var with fl32(var + eps) == 1.0, so that the folded BatchNorm scale is exactly gamma"""
    e = np.float32(eps)
    v = np.float32(1.0) - e
    for _ in range(8):
        if np.float32(v + e) == np.float32(1.0):
            return float(v)
        v = np.nextafter(v, np.float32(2.0 if np.float32(v + e) < 1.0 else 0.0), dtype=np.float32)
    raise AssertionError("no float32 var with fl32(var + eps) == 1")


def probe_columns(cin):
    """(column, sign) of the single input column that U', V' and R of channel c select at layer 0 (deeper layers carry
    attr[c mod 4] only, the same in every group of four)"""
    c = np.arange(C)
    g = c // 8                         # no two 8-channel groups select alike: a swap of two groups at a store shows
    return (((c + g) % cin, np.where((c + g) % 2 == 0, 1.0, -1.0)),
            ((3 * c + 1 + g // 2) % cin, np.where((c // 2 + g) % 2 == 0, 1.0, -1.0)), ((c + 2 + 3 * g) % cin, np.ones(C)))


def attr_probe_weights():
    """Wc4f of the e_attr (hi, lo) variant: small odd integers, every row different"""
    c = np.arange(C)[:, None]
    j = np.arange(4)[None, :]
    return (1 + 2 * ((c + 3 * j + (c // 4)) % 4)).astype(np.float32)


def set_probe_state_(model, kind):
    """Overwrite, through the state dict, the conv parameters of `model` (any SparseCADGCN with the reference's keys) so
    that after folding  s1 == 1, uv_shift == 0, t2f == 0, W2f == I, br == 0  and
        kind "count":  Wc4f[c] = e_(c mod 4);  layer 0: Wuv / Wr select single input columns (probe_columns) with +-1,
                       deeper layers: Wuv = Wr = 0
        kind "attr":   Wc4f = attr_probe_weights(), Wuv = Wr = 0 at every layer
    The node branch (mlp_node) keeps its values."""
    var = unit_running_var()
    sd = model.state_dict()
    prefixes = sorted({k[:k.index(".gconv.") + 7] for k in sd if ".gconv." in k},
                      key=lambda p: (0, 0) if ".head." in p else (1, int(p.split("backbone.")[1].split(".")[0])))
    for l, pre in enumerate(prefixes):
        cin = sd[pre + "lin_r.weight"].shape[1]
        W1 = torch.zeros(C, 2 * cin + 4)
        Wr = torch.zeros(C, cin)
        if kind == "count":
            W1[torch.arange(C), 2 * cin + torch.arange(C) % 4] = 1.0
            if l == 0:
                (cu, su), (cv, sv), (cr, sr) = probe_columns(cin)
                for c in range(C):
                    W1[c, cin + cv[c]] += sv[c]                  # W1b: V' = W1b x_src
                    W1[c, cv[c]] += sv[c]                        # W1a = W1b + (the U' selector): U' = (W1a - W1b) x_dst
                    W1[c, cu[c]] += su[c]
                    Wr[c, cr[c]] = sr[c]
        elif kind == "attr":
            W1[:, 2 * cin:] = torch.from_numpy(attr_probe_weights())
        else:
            raise ValueError(kind)
        new = {"nn.0.weight": W1, "nn.0.bias": torch.zeros(C), "nn.3.weight": torch.eye(C), "nn.3.bias": torch.zeros(C),
               "lin_r.weight": Wr, "lin_r.bias": torch.zeros(C)}
        for bn in ("nn.1.", "nn.4."):
            new.update({bn + "weight": torch.ones(C), bn + "bias": torch.zeros(C), bn + "running_mean": torch.zeros(C),
                        bn + "running_var": torch.full((C,), var)})
        for k, v in new.items():
            sd[pre + k] = v.to(sd[pre + k].dtype)
    model.load_state_dict(sd)
    return model


def assert_probe_operands(ops, kind):
    """the folded operands read back from a plan (or fold_state) have the properties the probe's exactness rests on"""
    eye = torch.eye(C, dtype=torch.float64)
    for l, op in enumerate(ops):
        cin = op["Cin"]
        assert bool((op["s1"] == 1).all()) and bool((op["uv_scale"] == 1).all()), "s1 != 1 at layer %d" % l
        assert bool((op["uv_shift"] == 0).all()) and bool((op["t2f"] == 0).all()) and bool((op["br"] == 0).all()), l
        assert torch.equal(op["W2f"].double(), eye), "W2f is not the identity at layer %d" % l
        Wuv, Wr, Wc = op["Wuv"].double(), op["Wr"].double(), (op["Wc4"] * op["s1"][:, None]).double()
        if kind == "count":
            assert torch.equal(Wc, eye[torch.arange(C) % 4][:, :4]), "Wc4f[c] != e_(c mod 4) at layer %d" % l
            if l == 0:
                (cu, su), (cv, sv), (cr, sr) = probe_columns(cin)
                want = torch.zeros(3 * C, cin, dtype=torch.float64)
                for c in range(C):
                    want[c, cu[c]] = su[c]
                    want[C + c, cv[c]] = sv[c]
                    want[2 * C + c, cr[c]] = sr[c]
                assert torch.equal(torch.cat([Wuv, Wr]), want), "layer-0 selectors"
            else:
                assert bool((Wuv == 0).all()) and bool((Wr == 0).all()), l
        else:
            assert torch.equal(Wc, torch.from_numpy(attr_probe_weights()).double())
            assert bool((Wuv == 0).all()) and bool((Wr == 0).all()), l


def _bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16)


def count_probe_expected(x, attr_csr, g, cin, L):
    """Expected f rows of the "count" probe, per layer, as bfloat16: every operand is a small integer, so every stored
    intermediate and every sum is exact in fp32 in any order, and
        f = bf16(fl32(fma(sum m, fl32(1 / max(deg, 1)), R)))
    layer 0: m[c] = relu(+-x[dst, cu] +- x[src, cv] + attr[c mod 4]), R[c] = x[., cr]; deeper layers: m[c] = attr[c mod 4],
    R = 0.  Evaluated in float64, where sum m (< 2^15) times the fp32 reciprocal plus R is exact, then rounded ONCE to
    fp32 (the fma) and once to bfloat16."""
    x, a = x.double(), attr_csr.double()
    assert float(x.abs().max()) <= 8 and bool((x == x.round()).all()) and bool((a == a.round()).all())
    assert float(a.min()) >= 0 and float(a.max()) <= 7
    (cu, su), (cv, sv), (cr, sr) = probe_columns(cin)
    a64 = a[:, torch.arange(C) % 4]
    inv = (1.0 / g.deg.clamp(min=1).float()).double()[:, None]
    out = []
    for l in range(L):
        if l == 0:
            U = x[:, torch.from_numpy(cu)] * torch.from_numpy(su)
            V = x[:, torch.from_numpy(cv)] * torch.from_numpy(sv)
            R = x[:, torch.from_numpy(cr)] * torch.from_numpy(sr)
            m = torch.relu(U[g.dst] + V[g.src] + a64)
        else:
            R = torch.zeros(g.N, C, dtype=torch.float64)
            m = a64
        agg = torch.zeros(g.N, C, dtype=torch.float64).index_add(0, g.dst, m)
        assert float(agg.max()) < 2 ** 15 if agg.numel() else True
        out.append((agg * inv + R).float().to(torch.bfloat16))
    return out


def attr_probe_expected(attr_csr, g):
    """The e_attr (hi, lo) variant (in-degree 1 everywhere, Wuv = Wr = 0, Wc4f small odd integers = their own bf16, so
    the kernel forms sum_j w_j (a_hi + a_lo)_j): (want bf16 [N,64], keep [N,64] bool, float64 value).
    hi + lo is within 2^-17 |a| of a (SPLIT3's derivation) and all terms are positive, so the kernel's fp32 value is
    within (2^-17 + 6 2^-24) < 2^-16 relative of v = sum w a; h1, m and f re-round the same bf16 value.  f therefore
    EQUALS bf16(v) wherever v is further than 2^-16 |v| from a bf16 rounding midpoint; the other elements are left
    out (keep False): 2 2^-16 / 2^-8 = 0.8 % of a binade at its lower end, half that at its upper end."""
    a = attr_csr.double()
    assert bool((g.deg == 1).all()) and float(a.min()) > 0
    W = torch.from_numpy(attr_probe_weights()).double()
    v = torch.zeros(g.N, C, dtype=torch.float64).index_add(0, g.dst, a @ W.t())
    u = br.ulp_bf16(v)
    frac = v / u - torch.floor(v / u)                    # position inside the bf16 cell, in spacings
    keep = (frac - 0.5).abs() * u > 2.0 ** -16 * v
    return br.bf(v).to(torch.bfloat16), keep, v


def probe_mismatches(feats, expected, keep=None):
    """The probes' assertion: per layer, the number of stored bfloat16 elements that are not the expected number (a NaN
    never is; +0 and -0 are the same number), among the elements `keep` selects.  expected: a list per layer, or ONE
    tensor every layer must equal."""
    L = feats.shape[1] // C
    out = []
    for l in range(L):
        want = expected[l] if isinstance(expected, (list, tuple)) else expected
        bad = ~(feats[:, C * l:C * (l + 1)].float() == want.float())
        out.append(int((bad & keep).sum()) if keep is not None else int(bad.sum()))
    return out


# ---------------------------------------------------------------------------------------------
# layouts (structure only: edge [E,2] = (src, dst) int64 grouped by proposal, bbox_idx [N], P, g0)
# ---------------------------------------------------------------------------------------------
class _Builder(object):
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n, self.p = 0, 0
        self.bb, self.edges = [], []

    def empty_id(self):
        self.p += 1

    def add(self, n, dst=None, src=None):
        """a proposal of n nodes with in-edges at the (proposal-local) destinations dst; sources uniform unless given"""
        dst = np.zeros(0, np.int64) if dst is None else np.asarray(dst, np.int64)
        if src is None:
            src = self.rng.integers(0, n, dst.shape[0])
        assert dst.shape[0] == 0 or (dst.max() < n and src.max() < n)
        self.edges.append(np.stack([np.asarray(src, np.int64) + self.n, dst + self.n], 1))
        self.bb.append(np.full(n, self.p, np.int64))
        self.n += n
        self.p += 1

    def add_degrees(self, degs):
        self.add(len(degs), np.repeat(np.arange(len(degs)), degs))

    def finish(self, name, g0=0):
        edge = np.concatenate(self.edges, 0) if self.edges else np.zeros((0, 2), np.int64)
        return dict(name=name, edge=edge, bbox_idx=np.concatenate(self.bb), N=self.n, P=self.p, g0=g0)


def layout(name, NW, seed=0):
    """The layouts of the element-wise tests, the smallest that reach each limit of a T = 16 NW node / ET = 128 NW edge
    tile.  Names: LAYOUTS (flag 0) and FLAG_LAYOUTS (the flag is raised; outputs are not examined)."""
    T, ET = 16 * NW, 128 * NW
    b = _Builder(seed + 1000 * NW)
    rng = b.rng
    g0 = 0
    if name == "hub":                      # one node receives all ET edges: first, last, slot 15 of a stream
        for h in (0, T - 1, 31):
            b.add(T, np.full(ET, h))
    elif name in ("exact_fit", "flag_nodes", "flag_edges"):
        g0 = 64
        n = T + (name == "flag_nodes")
        e = ET + (name == "flag_edges")
        b.add(n, rng.integers(0, n, e))    # exactly T nodes / ET edges
        b.add(1)                           # one node, no edges
        for _ in range(5):                 # T/2-node proposals: two share a tile
            b.add(T // 2, rng.integers(0, T // 2, 3 * T // 2))
        for _ in range(3):                 # T/2 + 1: they cannot
            b.add(T // 2 + 1, rng.integers(0, T // 2 + 1, 2 * T))
    elif name == "ladder":                 # rows end at every offset of a 16-edge step
        b.add_degrees(np.arange(32))
        b.add_degrees([15, 16, 17, 31, 32, 33])
        b.add_degrees(np.arange(32)[::-1].copy())
        b.add_degrees([0, 33, 0, 32, 31, 0, 17, 16, 15, 1])
    elif name == "skewed":                 # all edges on the last / first 16 nodes: the <= 16-nodes clamp binds
        for n in sorted({64, T}):
            b.add_degrees(np.concatenate([np.zeros(n - 16, np.int64), rng.integers(12, 28, 16)]))
            b.add_degrees(np.concatenate([rng.integers(12, 28, 16), np.zeros(n - 16, np.int64)]))
    elif name == "singles":                # 64 one-node proposals with self-loops in one tile
        g0 = 64
        for i in range(64):
            b.add(1, np.zeros(1 + i % 3, np.int64))
        b.add(1)
    elif name.startswith("groups"):        # P = 64 k + 1 with g0 = 64 | 4 | 1; ids without nodes; nodes without edges
        g0 = int(name[6:])
        for p in range(129):
            if p in (40, 128):
                b.empty_id()               # an id without nodes, in the middle and at the end
            elif p == 60:
                b.add(T)                   # a whole tile without edges while E > 0
            elif 20 <= p < 26 or p % 7 == 3:
                b.add(int(rng.integers(1, 6)))
            else:
                n = int(rng.integers(1, 7))
                b.add(n, rng.integers(0, n, int(rng.integers(1, 3 * n + 1))))
    elif name == "chain":                  # in-degree 1 everywhere (the e_attr variant)
        for n in (T, 1, 7, T // 2, T // 2, 33, 5, T - 1, 2):
            b.add(n, np.arange(n), (np.arange(n) - 1) % n)
    else:
        raise ValueError(name)
    return b.finish(name, g0)


LAYOUTS = ("hub", "exact_fit", "ladder", "skewed", "singles", "groups64", "groups4", "groups1")
FLAG_LAYOUTS = ("flag_nodes", "flag_edges")


def shuffle_inside_proposals(lay, seed):
    """the same layout with every proposal's edges in random order (still grouped by proposal): (layout, perm)"""
    rng = np.random.default_rng(seed)
    owner = lay["bbox_idx"][lay["edge"][:, 1]]
    perm = np.argsort(owner + rng.random(owner.shape[0]) * 0.5, kind="stable")
    out = dict(lay)
    out["edge"] = lay["edge"][perm]
    return out, perm


def inputs(lay, cin, kind, seed=0):
    """(x [N,cin], e_attr [E,4]) fp32 tensors.  "normal": standard normal in every column, e_attr dense of order 1;
    "codes": integers, x in -8..8 and e_attr in 0..7 (the counting probe); "mantissa": e_attr in [0.5, 2) with full
    fp32 mantissas (the (hi, lo) variant)."""
    g = torch.Generator().manual_seed(seed * 7919 + cin)
    N, E = lay["N"], lay["edge"].shape[0]
    if kind == "normal":
        return torch.randn(N, cin, generator=g), torch.randn(E, 4, generator=g)
    if kind == "codes":
        return (torch.randint(-8, 9, (N, cin), generator=g).float(), torch.randint(0, 8, (E, 4), generator=g).float())
    if kind == "mantissa":
        return torch.randn(N, cin, generator=g), (torch.rand(E, 4, generator=g, dtype=torch.float64) * 1.5 + 0.5).float()
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------
# CPU emulation of the kernel's stated roundings, with named defects
# ---------------------------------------------------------------------------------------------
DEFECTS = ("drop_last_edge", "step_first_to_prev_slot", "skip_partial_step", "deg_plus_one", "swap_gathers",
           "ignore_x_col0", "drop_attr_lo", "swap_channel_groups", "mean_cnt_plus_one")


def _b(t):
    return t.to(torch.bfloat16).float()


def _hi_lo(t):
    hi = _b(t)
    return hi, _b(t - hi)


def emulate(ops, x, attr_csr, g, NW, g0=0, defect=None):
    """The kernel's arithmetic on the CPU: fp32 accumulation, bfloat16 at the six storage points, the (hi, lo) pairs with
    three cross terms, fl32(1 / deg) and one fma at the end.  ops: fold_state(model) (fp32).  Returns (feats [N, 64 L]
    bfloat16, Zmean [P, 64 L] fp32, flag).  defect (DEFECTS) plants one named error:
        drop_last_edge            the last in-edge of every row is not summed
        step_first_to_prev_slot   the first edge of every 16-edge step of a stream goes to the previous node slot
        skip_partial_step         a stream's final partial step is not summed
        deg_plus_one              the mean divides by deg + 1
        swap_gathers              U' is gathered at src and V' at dst
        ignore_x_col0             layer 0's node phase skips input column 0
        drop_attr_lo              e_attr enters as its hi half only
        swap_channel_groups       channels 8..15 and 24..31 trade places at the store of f
        mean_cnt_plus_one         the pooled mean of s divides by cnt + 1"""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x, attr = x.float(), attr_csr.float()
    tiles, flag = tile_plan(g, NW, g0)
    dst, src, E = g.dst, g.src, g.E
    tgt, keep = dst.clone(), torch.ones(E, dtype=torch.bool)
    if defect == "drop_last_edge":
        keep[(g.row_ptr[1:] - 1)[g.deg > 0]] = False
    for t in tiles:
        for j in range(2 * NW):
            a, b_ = t["ns"][j], t["ns"][j + 1]
            e_a, e_b = int(g.row_ptr[t["n0"] + a]), int(g.row_ptr[t["n0"] + b_])
            if defect == "step_first_to_prev_slot":
                for e in range(e_a, e_b, 16):
                    if int(dst[e]) - t["n0"] > a:
                        tgt[e] = dst[e] - 1
            if defect == "skip_partial_step" and (e_b - e_a) % 16:
                keep[e_b - (e_b - e_a) % 16:e_b] = False
    deg = g.deg.float()
    inv = 1.0 / ((deg + 1.0) if defect == "deg_plus_one" else deg.clamp(min=1.0))
    ah, al = _hi_lo(attr)
    if defect == "drop_attr_lo":
        al = torch.zeros_like(al)
    feats, zmean = [], []
    fin, sin = x, x
    for l, op in enumerate(ops):
        W32 = torch.cat([op["Wuv"] * op["uv_scale"][:, None], op["Wr"], op["Wn"] * op["sn"][:, None]], 0).float()
        shift = torch.cat([op["uv_shift"], op["br"], op["bn"] * op["sn"] + op["tn"]]).float()
        if l == 0:
            xin = x.clone()
            if defect == "ignore_x_col0":
                xin[:, 0] = 0.0
            xh, xl = _hi_lo(xin)
            wh, wl = _hi_lo(W32)
            out = shift + (xh @ wh.t() + xl @ wh.t() + xh @ wl.t())
        else:
            Wb = _b(W32)
            out = shift + torch.cat([fin @ Wb[:3 * C].t(), sin @ Wb[3 * C:].t()], 1)
        U, V, R, s = _b(out[:, :C]), _b(out[:, C:2 * C]), out[:, 2 * C:3 * C], torch.relu(_b(out[:, 3 * C:]))
        wch, wcl = _hi_lo((op["Wc4"] * op["s1"][:, None]).float())
        gu, gv = (src, dst) if defect == "swap_gathers" else (dst, src)
        z = U[gu] + V[gv] + (ah @ wch.t() + al @ wch.t() + ah @ wcl.t())
        h1 = torch.relu(_b(z))
        m = torch.relu(_b(h1 @ op["W2f"].float().t() + op["t2f"].float()))
        agg = torch.zeros(g.N, C).index_add(0, tgt[keep], m[keep])
        f = (agg.double() * inv.double()[:, None] + R.double()).float().to(torch.bfloat16)     # one fma, one store
        if defect == "swap_channel_groups":
            f = torch.cat([f[:, 0:8], f[:, 24:32], f[:, 16:24], f[:, 8:16], f[:, 32:]], 1)
        cnt = g.cnt.float() + (1.0 if defect == "mean_cnt_plus_one" else 0.0)
        zm = torch.zeros(g.P, C).index_add(0, g.bbox_idx, s) * (1.0 / cnt.clamp(min=1.0))[:, None]
        feats.append(f)
        zmean.append(zm)
        fin, sin = f.float(), s
    return torch.cat(feats, 1), torch.cat(zmean, 1), flag
