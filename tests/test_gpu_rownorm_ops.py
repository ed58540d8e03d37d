"""Op-level tests of csrc/rownorm.hip per element against float64.

  yolat_rownorm_act / yolat_rownorm_act_bwd      Z = relu?(rownorm(Y) gamma + beta) and its backward: C in {256, 512, 1024, 100}
                                                 and {1100, 2048} (the instantiations that re-read the row per pass),
                                                 M in {1, 63, 64, 65, 300}, gamma / beta present and NULL, ReLU on and off, in
                                                 place and out of place.  Rows: N(0,1), rows offset by +10 and by +100 (a
                                                 variance taken as E[y^2] - mean^2 is wrong by 1.4e-3 of the largest output
                                                 there), one constant row (must give exactly beta).
  yolat_fusion_pair_eval_x6_rn / _rn             Linear -> row norm -> ReLU -> per-proposal max (and the stored super half),
                                                 the fused kernel (D = 128, 64) and the materialising route (D = 32, and D = 64
                                                 on the same input), F = 1024; N in {1, R - 1, R, R + 1, 2 R + 3} with R = the
                                                 fused kernel's 128 rows per workgroup, one-node proposals, a proposal across
                                                 a row-tile edge, one longer than a tile, proposals without rows, P = 1, and
                                                 the layouts of segmax_layouts.py; one case with the bias shifted until
                                                 |row mean| / row std >= 30.

Bars.  Forward: |z - ref| <= 1e-4 * max|ref| per element.  Backward: the project's gradient rule, 1e-3 * max|g_ref| +
2e-5 * gmax per tensor, and the same bound per element of dY; the constant row (rstd = 1 / sqrt(eps) = 316: its gradients are
300 times everybody else's) is held to its own maximum and left out of the other rows' maximum, which only tightens the rule.
Elements whose float64 pre-activation lies within 1e-5 * max|pre| of zero are left out of the dY comparison (the ReLU gate of
an fp32 kernel may fall on the other side there); the tests assert that they are <= 0.5 % of the elements.  The constant row
takes no such exclusion: its pre-activation is exactly beta (exactly 0 without gamma / beta: gate closed, as torch's) on both
sides.

Reference margin, checked on the CPU by the two tests below that carry no gpu mark: torch's own fp32 LayerNorm / autograd on
the same inputs sits within a tenth of every bar (measured: forward 3.3e-6 of the maximum against the bar's 1e-4, the +100
rows included; gradients 0.7 % of their bound; the fusion pair in fp32 2.4e-6 of the maximum against its 1e-4, the shifted
bias included).  The kernels, on the MI355X: the fusion pair <= 5e-7 (fused) and <= 7.3e-7 (materialising) of the maximum."""
import functools

import numpy as np
import pytest
import torch

import segmax_layouts as sl

gpu = pytest.mark.gpu

EPS = 1e-5
TOL_FWD = 1e-4
CS = (256, 512, 1024, 100, 1100, 2048)       # 1100, 2048: beyond the 1024 columns a wave keeps in registers (the row is re-read)
MS = (1, 63, 64, 65, 300)
KINDS = ("normal", "plus10", "plus100", "constant")
COMBOS = [(affine, relu) for affine in (True, False) for relu in (True, False)]


def _rows(M, C, seed, kind=None):
    """[M, C] rows from N(0,1); M >= 4: row 1 (and every 7th) offset by +10, row 2 (and every 11th) by +100, row 3 constant.
    M == 1: the one row is of `kind`."""
    tg = torch.Generator().manual_seed(seed)
    y = torch.randn(M, C, generator=tg)
    const = []
    if M == 1:
        if kind == "plus10":
            y += 10.0
        elif kind == "plus100":
            y += 100.0
        elif kind == "constant":
            y[:] = 3.7
            const = [0]
    else:
        y[1::7] += 10.0
        y[2::11] += 100.0
        y[3] = 3.7
        const = [3]
    return y, const


@functools.lru_cache(maxsize=None)
def _case(M, C, affine, relu, kind=None):
    """Inputs and the float64 reference (forward, pre-activation, gradients) of one case — computed once, read only."""
    y, const = _rows(M, C, 1000 * C + M + (KINDS.index(kind) if kind else 0), kind)
    tg = torch.Generator().manual_seed(7 * C + M)
    gz = torch.randn(M, C, generator=tg)
    gamma = (torch.rand(C, generator=tg) + 0.5) if affine else None
    beta = (torch.randn(C, generator=tg) * 0.3) if affine else None
    y64 = y.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True) if affine else None
    b64 = beta.double().requires_grad_(True) if affine else None
    mean, var = y64.mean(1, keepdim=True), y64.var(1, unbiased=False, keepdim=True)
    pre = (y64 - mean) / torch.sqrt(var + EPS)
    if affine:
        pre = pre * g64 + b64
    z = torch.relu(pre) if relu else pre
    (z * gz.double()).sum().backward()
    grads = {"dY": y64.grad}
    if affine:
        grads.update(dgamma=g64.grad, dbeta=b64.grad)
    return dict(y=y, gz=gz, gamma=gamma, beta=beta, const=const, z=z.detach(), pre=pre.detach(), grads=grads)


def _check_forward(tag, got, c):
    want = c["z"]
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.double() - want).abs().max())
    print("%s forward: %.2e of %.3g" % (tag, err / scale, scale))
    assert err <= TOL_FWD * scale, tag
    return err / scale


def _check_backward(tag, got, c, relu):
    """got: dict like c["grads"].  Returns the worst error as a fraction of its bound."""
    ref = c["grads"]
    M = c["y"].shape[0]
    const = torch.zeros(M, dtype=torch.bool)
    const[c["const"]] = True
    worst = 0.0
    for rows in (const, ~const):
        if not bool(rows.any()):
            continue
        # parameter gradients are sums over all rows, and the constant row adds nothing unusual to them (xh = 0, g = dZ): they
        # are held to the ordinary rows' gmax (a case of one constant row alone has nothing else)
        with_params = rows is not const or bool(const.all())
        tensors = {"dY": (got["dY"].double()[rows], ref["dY"][rows])}
        if with_params:
            for k in ("dgamma", "dbeta"):
                if k in ref:
                    tensors[k] = (got[k].double(), ref[k])
        gmax = max(float(w.abs().max()) for _, w in tensors.values())
        for k, (g, w) in tensors.items():
            bound = 1e-3 * float(w.abs().max()) + 2e-5 * gmax
            diff = (g - w).abs()
            if k == "dY" and relu and rows is not const:
                # (the constant row takes no exclusion: its pre-activation is exactly beta, or exactly 0, on both sides)
                pre = c["pre"][rows]
                kink = pre.abs() <= 1e-5 * float(c["pre"].abs().max())
                share = float(kink.double().mean())
                assert share <= 0.005, (tag, share)
                diff = diff[~kink]
            err = float(diff.max()) if diff.numel() else 0.0
            print("%s %s%s: %.2e of bound %.3g" % (tag, k, " (constant row)" if rows is const else "", err, bound))
            assert err <= bound, (tag, k)                 # per tensor and, for dY, per element: the same number
            worst = max(worst, err / max(bound, 1e-30))
    return worst


def _cases():
    for C in CS:
        for M in MS:
            for kind in (KINDS if M == 1 else (None,)):
                yield M, C, kind


def test_cpu_fp32_reference_sits_within_a_tenth_of_the_row_norm_bars():
    worst_f = worst_b = 0.0
    for M, C, kind in _cases():
        for affine, relu in COMBOS:
            c = _case(M, C, affine, relu, kind)
            y = c["y"].clone().requires_grad_(True)
            ga = c["gamma"].clone().requires_grad_(True) if affine else None
            be = c["beta"].clone().requires_grad_(True) if affine else None
            pre = torch.nn.functional.layer_norm(y, (C,), ga, be, EPS)
            z = torch.relu(pre) if relu else pre
            (z * c["gz"]).sum().backward()
            tag = "cpu M=%d C=%d %s affine=%d relu=%d" % (M, C, kind, affine, relu)
            worst_f = max(worst_f, _check_forward(tag, z.detach(), c))
            got = {"dY": y.grad}
            if affine:
                got.update(dgamma=ga.grad, dbeta=be.grad)
            worst_b = max(worst_b, _check_backward(tag, got, c, relu))
    print("torch fp32 on the CPU: forward %.2e of the maximum, backward %.2e of its bound" % (worst_f, worst_b))
    assert worst_f <= 0.1 * TOL_FWD and worst_b <= 0.1


@gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("C", CS)
def test_rownorm_act_forward_and_backward_vs_fp64(C, M):
    from yolat_vectorgraphicsrecognition_amd import ops
    for kind in (KINDS if M == 1 else (None,)):
        for affine, relu in COMBOS:
            c = _case(M, C, affine, relu, kind)
            tag = "M=%d C=%d %s affine=%d relu=%d" % (M, C, kind, affine, relu)
            yd, gzd = c["y"].cuda(), c["gz"].cuda()
            ga = c["gamma"].cuda() if affine else None
            be = c["beta"].cuda() if affine else None
            stats = torch.empty(2, M, device="cuda")
            z = ops.rownorm_act(yd, ga, be, EPS, relu, torch.full_like(yd, float("nan")), stats[0], stats[1])
            buf = yd.clone()
            zin = ops.rownorm_act(buf, ga, be, EPS, relu, buf)                    # in place, nothing saved
            assert torch.equal(z, zin), tag
            # a strided destination / source (a column slice of a wider buffer, as the engine's Z[:, F + D:2 F + D])
            wide = torch.full((M, C + 24), float("nan"), device="cuda")
            wide[:, 8:8 + C] = yd
            ops.rownorm_act(wide[:, 8:8 + C], ga, be, EPS, relu, wide[:, 8:8 + C])
            assert torch.equal(wide[:, 8:8 + C], z) and bool(torch.isnan(wide[:, :8]).all()) and bool(torch.isnan(wide[:, 8 + C:]).all())
            _check_forward(tag, z.cpu(), c)
            for r in c["const"]:
                want = (c["beta"] if affine else torch.zeros(C))
                want = torch.relu(want) if relu else want
                assert torch.equal(z[r].cpu(), want), tag                        # exactly beta
            mean64 = c["y"].double().mean(1)
            assert float((stats[0].cpu().double() - mean64).abs().max()) <= 1e-6 * max(float(mean64.abs().max()), 1.0), tag

            def run(inplace):
                dg = torch.full((C,), float("nan"), device="cuda") if affine else None
                db = torch.full((C,), float("nan"), device="cuda") if affine else None
                dz = gzd.clone()
                dy = ops.rownorm_act_bwd(dz, yd, stats[0], stats[1], ga, be, relu, dg, db, dz if inplace else torch.empty_like(yd))
                out = {"dY": dy}
                if affine:
                    out.update(dgamma=dg, dbeta=db)
                return out
            got, again, inpl = run(False), run(False), run(True)
            for k in got:
                assert torch.equal(got[k], again[k]), (tag, k)                    # two calls: identical bits
                assert torch.equal(got[k], inpl[k]), (tag, k)                     # dY written over dZ: the same
            _check_backward(tag, {k: v.cpu() for k, v in got.items()}, c, relu)


# ---- the fusion pair -------------------------------------------------------------------------------------------------
R = 128                 # YOLAT_RN_ROWS (tests/test_norm_host.py pins ops.RN_ROWS to it)
F = 1024


def _layout(name):
    if name == "n1":
        return sl._from_sizes(name, [1])                                   # N = 1, P = 1
    if name == "ones_r-1":
        return sl._from_sizes(name, [1] * (R - 1))                         # one-node proposals, N = R - 1
    if name == "empty_r":
        return sl._from_sizes(name, [0, 60, 0, 0, 68, 0])                  # proposals without rows, N = R
    if name == "straddle_r+1":
        return sl._from_sizes(name, [120, 9])                              # a proposal across the row-tile edge, N = R + 1
    if name == "long_2r+3":
        return sl._from_sizes(name, [2 * R + 3])                           # P = 1, longer than a tile (three tiles)
    return sl.layout(name)


LAYOUTS = ("n1", "ones_r-1", "empty_r", "straddle_r+1", "long_2r+3", "straddle", "tiny_then_long", "empty")


@functools.lru_cache(maxsize=None)
def _pair_case(name, D, affine, shift=0.0):
    lay = _layout(name)
    N, P = lay.N, lay.P
    tg = torch.Generator().manual_seed(13 * LAYOUTS.index(name) + D + int(shift))
    A = torch.relu(torch.randn(N, D, generator=tg)) + 0.3 * torch.rand(1, D, generator=tg)
    S = torch.randn(P, D, generator=tg)
    Wf, Wfs = torch.randn(F, D, generator=tg) / D ** 0.5, torch.randn(F, D, generator=tg) / D ** 0.5
    bf, bfs = torch.randn(F, generator=tg) * 0.1 + shift, torch.randn(F, generator=tg) * 0.1 - shift
    gb = [(torch.rand(F, generator=tg) + 0.5, torch.randn(F, generator=tg) * 0.3) if affine else (None, None) for _ in range(2)]

    def block(X, W, b, g, dt):
        y = X.to(dt) @ W.to(dt).t() + b.to(dt)
        z = torch.nn.functional.layer_norm(y, (F,), None if g[0] is None else g[0].to(dt), None if g[1] is None else g[1].to(dt), EPS)
        return torch.relu(z), y

    def pooled(dt):
        z, y = block(A, Wf, bf, gb[0], dt)
        out = torch.zeros(P, F, dtype=dt)
        out.index_reduce_(0, torch.from_numpy(lay.bbox_idx), z, "amax", include_self=False)
        out[torch.from_numpy(lay.sizes == 0)] = 0.0
        return out, y
    want, y = pooled(torch.float64)
    ratio = float((y.mean(1).abs() / y.std(1, unbiased=False)).min())
    return dict(lay=lay, A=A, S=S, Wf=Wf, Wfs=Wfs, bf=bf, bfs=bfs, gb=gb, want=want, want_s=block(S, Wfs, bfs, gb[1], torch.float64)[0],
                fp32=(pooled(torch.float32)[0], block(S, Wfs, bfs, gb[1], torch.float32)[0]), ratio=ratio)


PAIR_CASES = [(name, D, 0.0) for name in LAYOUTS for D in (128, 64, 32)] + [("straddle_r+1", D, 40.0) for D in (128, 64, 32)]


def test_cpu_fp32_oracle_sits_within_a_tenth_of_the_fusion_pair_bar():
    worst = 0.0
    for name, D, shift in PAIR_CASES:
        for affine in (True, False):
            c = _pair_case(name, D, affine, shift)
            for got, want in zip(c["fp32"], (c["want"], c["want_s"])):
                worst = max(worst, float((got.double() - want).abs().max()) / float(want.abs().max()))
    print("fp32 oracle: %.2e of the maximum" % worst)
    assert worst <= 0.1 * TOL_FWD
    assert _pair_case("straddle_r+1", 128, True, 40.0)["ratio"] >= 30.0


@gpu
@pytest.mark.parametrize("name,D,shift", PAIR_CASES)
def test_fusion_pair_rownorm_vs_fp64(name, D, shift):
    """D = 128 / 64: the fused kernel; D = 32: the materialising route; D = 64: both, on the same input."""
    from yolat_vectorgraphicsrecognition_amd import ops
    for affine in (True, False):
        c = _pair_case(name, D, affine, shift)
        lay = c["lay"]
        P = lay.P
        if shift:
            assert c["ratio"] >= 30.0
        dev = {k: c[k].cuda() for k in ("A", "S", "Wf", "Wfs", "bf", "bfs")}
        lin_f, lin_s = torch.nn.Linear(D, F), torch.nn.Linear(D, F)
        with torch.no_grad():
            lin_f.weight.copy_(c["Wf"]); lin_f.bias.copy_(c["bf"]); lin_s.weight.copy_(c["Wfs"]); lin_s.bias.copy_(c["bfs"])
        lin_f, lin_s = lin_f.cuda(), lin_s.cuda()
        gb = [tuple(None if t is None else t.cuda() for t in g) for g in c["gb"]]
        seg = torch.from_numpy(lay.bbox_idx).int().cuda()
        ZW = 2 * (F + D)
        routes = [("fused", ops.fusion_pair_eval_x6_rn)] if D in (64, 128) else []
        if D in (32, 64):
            routes.append(("generic", ops.fusion_pair_eval_rn))
        empty = torch.from_numpy(lay.sizes == 0)
        for tag, fn in routes:
            outs = []
            for _ in range(2):
                Z = torch.full((P, ZW), float("nan"), device="cuda")
                Z[:, :F] = 0.0                                           # the pooled block is merged by atomicMax: zero-filled
                fn(dev["A"], lin_f, gb[0], seg, Z[:, :F], dev["S"], lin_s, gb[1], Z[:, F + D:2 * F + D], EPS)
                outs.append(Z)
            torch.cuda.synchronize()
            assert torch.equal(outs[0][:, :F], outs[1][:, :F]) and torch.equal(outs[0][:, F + D:2 * F + D], outs[1][:, F + D:2 * F + D])
            Zt = outs[0].cpu()
            assert bool(torch.isnan(Zt[:, F:F + D]).all()) and bool(torch.isnan(Zt[:, 2 * F + D:]).all()), tag   # not written
            err = float((Zt[:, :F].double() - c["want"]).abs().max()) / float(c["want"].abs().max())
            err_s = float((Zt[:, F + D:2 * F + D].double() - c["want_s"]).abs().max()) / float(c["want_s"].abs().max())
            print("rownorm pair %s D=%d %s affine=%d shift %g: pooled %.2e super %.2e" % (tag, D, name, affine, shift, err, err_s))
            assert err <= TOL_FWD and err_s <= TOL_FWD, tag
            if bool(empty.any()):
                assert float(Zt[empty, :F].abs().max()) == 0.0, tag
