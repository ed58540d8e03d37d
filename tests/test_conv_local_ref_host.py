"""Host checks (no GPU) of tests/conv_local_ref.py, the reference of tests/test_gpu_conv_local_elements.py: the float64
want is the oracle's Backbone, a CPU emulation of the kernel's stated roundings passes every assertion the GPU test makes
on every layout, each named defect planted in that emulation is rejected by the assertion aimed at it, the layouts reach
the tile limits they are named after, and the left-out share of the e_attr (hi, lo) variant stays within its cap."""
import functools

import numpy as np
import pytest
import torch

import conv_local_ref as cl
import golden_util as gu
from oracle import oracle_torch as orc

L = 4
CINS = (3, 5, 8)
LEFT_OUT_CAP = 0.02


@functools.lru_cache(maxsize=None)
def _model(cin, kind=None):
    m = gu.fill_state_(orc.SparseCADGCN(orc.Opt(n_classes=17, n_blocks=L, n_blocks_out=L, in_channels=cin)), 50 + cin).eval()
    return cl.set_probe_state_(m, kind) if kind else m


@functools.lru_cache(maxsize=None)
def _ops(cin, kind=None):
    return cl.fold_state(_model(cin, kind))


@functools.lru_cache(maxsize=None)
def _case(name, NW, cin, kind):
    """(layout, Csr, x, e_attr in CSR order) of a layout with inputs of `kind`"""
    lay = cl.layout(name, NW)
    g = cl.Csr(lay["edge"], lay["bbox_idx"], lay["N"], lay["P"])
    x, attr = cl.inputs(lay, cin, kind)
    return lay, g, x, attr[g.perm]


def _cin_of(name):
    return CINS[cl.LAYOUTS.index(name) % 3]


def test_unit_running_var_folds_to_scale_one():
    v = np.float32(cl.unit_running_var())
    assert np.float32(v + np.float32(1e-5)) == np.float32(1.0)
    assert np.float32(1.0) / np.sqrt(np.float32(v + np.float32(1e-5))) == np.float32(1.0)


def test_split3_bound_holds_for_random_pairs():
    """SPLIT3's derivation, tried: three cross terms of (hi, lo) pairs against the exact product"""
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(200000, generator=g) * torch.exp2(torch.randint(-6, 6, (200000,), generator=g).float()))
    x = (torch.randn(200000, generator=g) * torch.exp2(torch.randint(-6, 6, (200000,), generator=g).float()))
    wh, wl = cl._hi_lo(w)
    xh, xl = cl._hi_lo(x)
    got = wh.double() * xh.double() + wh.double() * xl.double() + wl.double() * xh.double()
    rel = (got - w.double() * x.double()).abs() / (w.double() * x.double()).abs().clamp(min=1e-300)
    assert float(rel.max()) <= cl.SPLIT3
    assert float(rel.max()) > 2.0 ** -18            # ... and the bound is not idle: the dropped term is really there
    assert float(((wh + wl).double() - w.double()).abs().div(w.double().abs().clamp(min=1e-300)).max()) <= 2.0 ** -17


@pytest.mark.parametrize("cin", CINS)
def test_unrounded_want_is_the_oracle_backbone_in_float64(cin):
    lay, g, x, _ = _case("ladder", 4, cin, "normal")
    _, attr = cl.inputs(lay, cin, "normal")
    model = _model(cin)
    fs, zs = cl.unrounded_forward(model, x, lay["edge"], attr, lay["bbox_idx"], lay["P"])
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(n_classes=17, n_blocks=L, n_blocks_out=L, in_channels=cin)), 50 + cin)
    ref = ref.double().eval()
    with torch.no_grad():
        out_feat, out_sup = ref.cls_net(x.double(), [torch.from_numpy(lay["edge"]).t()], [None], [attr.double()],
                                        torch.from_numpy(lay["bbox_idx"]))
    F = out_feat.shape[1] - 64 * L
    for name, got, want in (("f", torch.cat(fs, 1), out_feat[:, F:]), ("mean s", torch.cat(zs, 1), out_sup[:, F:])):
        # two float64 evaluations in different association (folded BatchNorm, factorised first Linear), four layers deep
        err = (got - want).abs()
        assert bool((err <= 1e-9 * (1.0 + want.abs())).all()), (name, float(err.max()))
    assert float(out_feat[:, F:].abs().max()) > 0.1


@pytest.mark.parametrize("NW", [4, 8])
@pytest.mark.parametrize("name", cl.LAYOUTS)
def test_layouts_reach_the_limits_they_are_named_after(name, NW):
    T, ET, NS = 16 * NW, 128 * NW, 2 * NW
    lay, g, _, _ = _case(name, NW, 5, "normal")
    tiles, flag = cl.tile_plan(g, NW, lay["g0"])
    assert flag == 0
    owner = lay["bbox_idx"][lay["edge"]]
    assert bool((owner[:, 0] == owner[:, 1]).all()) and bool((np.diff(owner[:, 1]) >= 0).all())      # local, grouped
    assert sum(t["nt"] for t in tiles) == g.N and sum(t["et"] for t in tiles) == g.E
    for t in tiles:
        assert t["ns"][0] == 0 and t["ns"][-1] == t["nt"] and all(0 <= b - a <= 16 for a, b in zip(t["ns"], t["ns"][1:]))
    deg = g.deg.numpy()
    if name == "hub":
        assert [(t["nt"], t["et"]) for t in tiles] == [(T, ET)] * 3
        hubs = np.flatnonzero(deg)
        assert list(hubs) == [0, 2 * T - 1, 2 * T + 31] and bool((deg[hubs] == ET).all())
        assert [int(h) % T % 16 for h in hubs] == [0, 15, 15]
    elif name == "exact_fit":
        assert (tiles[0]["nt"], tiles[0]["et"]) == (T, ET)
        assert [t["p1"] - t["p0"] for t in tiles] == [1, 2, 2, 2, 1, 1, 1]
        assert [t["nt"] for t in tiles] == [T, 1 + T // 2, T, T, T // 2 + 1, T // 2 + 1, T // 2 + 1]
        for bad in cl.FLAG_LAYOUTS:
            lb = cl.layout(bad, NW)
            assert cl.tile_plan(cl.Csr(lb["edge"], lb["bbox_idx"], lb["N"], lb["P"]), NW, lb["g0"])[1] == 1
    elif name == "ladder":
        assert list(deg[:32]) == list(range(32)) and list(deg[32:38]) == [15, 16, 17, 31, 32, 33]
        assert set(int(r) % 16 for r in g.row_ptr[1:33]) == set(range(16))
    elif name == "skewed":
        binds = [any(n != c for n, c in zip(t["ns"], t["cand"])) for t in tiles]
        assert all(binds) and len(tiles) >= 2
        assert bool((deg[:48] == 0).all()) and bool((deg[48:64] > 0).all())
    elif name == "singles":
        assert tiles[0]["p1"] - tiles[0]["p0"] == 64 and tiles[0]["nt"] == 64
        assert bool((lay["edge"][:, 0] == lay["edge"][:, 1]).all())
    else:
        assert lay["P"] == 129 and lay["P"] % lay["g0"] == 1 % lay["g0"]
        cnt = g.cnt.numpy()
        assert cnt[40] == 0 and cnt[128] == 0 and g.E > 0
        assert any(t["et"] == 0 and t["nt"] > 0 for t in tiles)
        assert any(t["nt"] == T and t["et"] == 0 for t in tiles)


@pytest.mark.parametrize("NW", [4, 8])
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("name", cl.LAYOUTS)
def test_emulation_lies_inside_the_envelope_on_every_layout(name, cin, NW):
    lay, g, x, attr = _case(name, NW, cin, "normal")
    ops = _ops(cin)
    feats, zmean, flag = cl.emulate(ops, x, attr, g, NW, lay["g0"])
    assert flag == 0
    pks = cl.pack_model(ops)
    for l, (ratio, n_out, where, _) in enumerate(cl.check_feats(feats, x, attr, pks, g)):
        assert n_out == 0, "layer %d: |err| / tol = %.3f at %s" % (l, ratio, where)
        assert ratio > 1e-3                      # the envelope is of the error's own order of magnitude
    for l, (ratio, n_out) in enumerate(cl.check_zmean(zmean, x, pks, g)):
        assert n_out == 0, "mean s, layer %d: %.3f" % (l, ratio)


@pytest.mark.parametrize("NW", [4, 8])
@pytest.mark.parametrize("name", cl.LAYOUTS)
def test_emulation_reproduces_the_counting_probe_bit_for_bit(name, NW):
    cin = _cin_of(name)
    lay, g, x, attr = _case(name, NW, cin, "codes")
    ops = _ops(cin, "count")
    cl.assert_probe_operands(ops, "count")
    feats, _, _ = cl.emulate(ops, x, attr, g, NW, lay["g0"])
    want = cl.count_probe_expected(x, attr, g, cin, L)
    assert cl.probe_mismatches(feats, want) == [0] * L
    assert all(float(w.float().abs().max()) > 0 for w in want)
    # the probe is inside the envelope as well (the two references agree with each other)
    assert all(r[1] == 0 for r in cl.check_feats(feats, x, attr, cl.pack_model(ops), g))


@pytest.mark.parametrize("NW", [4, 8])
def test_attr_variant_emulation_and_left_out_share(NW):
    lay, g, x, attr = _case("chain", NW, 5, "mantissa")
    ops = _ops(5, "attr")
    cl.assert_probe_operands(ops, "attr")
    want, keep, v = cl.attr_probe_expected(attr, g)
    left_out = 1.0 - float(keep.double().mean())
    assert 0.0 < left_out <= LEFT_OUT_CAP, left_out
    feats, _, _ = cl.emulate(ops, x, attr, g, NW, lay["g0"])
    assert cl.probe_mismatches(feats, want, keep) == [0] * L
    # full mantissas: the lo halves matter (without them a good share of the kept elements round the other way)
    assert float(((attr - attr.to(torch.bfloat16).float()) != 0).double().mean()) > 0.9


def _rejected_by(defect, NW):
    """run the emulation with `defect` on the layout aimed at it and return (what the GPU test's assertion sees, same
    without the defect)"""
    def envelope(name, cin):
        lay, g, x, attr = _case(name, NW, cin, "normal")
        pks = cl.pack_model(_ops(cin))
        out = []
        for d in (defect, None):
            feats, zmean, _ = cl.emulate(_ops(cin), x, attr, g, NW, lay["g0"], defect=d)
            out.append((sum(r[1] for r in cl.check_feats(feats, x, attr, pks, g)),
                        sum(n for _, n in cl.check_zmean(zmean, x, pks, g))))
        return out

    def count(name, cin):
        lay, g, x, attr = _case(name, NW, cin, "codes")
        want = cl.count_probe_expected(x, attr, g, cin, L)
        return [cl.probe_mismatches(cl.emulate(_ops(cin, "count"), x, attr, g, NW, lay["g0"], defect=d)[0], want)
                for d in (defect, None)]

    if defect in ("drop_last_edge", "step_first_to_prev_slot", "skip_partial_step", "deg_plus_one"):
        bad, good = count("ladder", 5)
        hub_bad, hub_good = count("hub", 3)            # one edge in ET = 128 NW: only the exact probe can see it
        assert hub_good == [0] * L
        if defect != "skip_partial_step":               # (the hub's streams end on full steps)
            assert all(n > 0 for n in hub_bad), hub_bad
        return bad, good
    if defect in ("swap_gathers", "ignore_x_col0"):
        bad, good = count("exact_fit", 8)
        assert good == [0] * L and bad[0] > 0           # the x gather path is layer 0's
        (fb, _), (fg, _) = envelope("exact_fit", 8)
        assert fb > 0 and fg == 0
        return bad[:1], good[:1]
    if defect == "swap_channel_groups":
        (fb, _), (fg, _) = envelope("exact_fit", 5)
        assert fb > 0 and fg == 0
        bad, good = count("exact_fit", 8)               # (deeper layers of the probe repeat every four channels)
        return bad[:1], good
    if defect == "mean_cnt_plus_one":
        (_, zb), (_, zg) = envelope("singles", 3)
        return [zb], [zg]
    if defect == "drop_attr_lo":
        lay, g, x, attr = _case("chain", NW, 5, "mantissa")
        want, keep, _ = cl.attr_probe_expected(attr, g)
        return [cl.probe_mismatches(cl.emulate(_ops(5, "attr"), x, attr, g, NW, lay["g0"], defect=d)[0], want, keep)
                for d in (defect, None)]
    raise AssertionError(defect)


@pytest.mark.parametrize("NW", [4, 8])
@pytest.mark.parametrize("defect", cl.DEFECTS)
def test_every_named_defect_is_rejected(defect, NW):
    bad, good = _rejected_by(defect, NW)
    assert all(n == 0 for n in good), good
    assert all(n > 0 for n in bad), bad


def test_shuffled_layouts_have_the_same_sorted_form():
    """the COO variants of the GPU test: the stable destination sort of a shuffled list visits a row's edges in another
    order, the reference (order-free) stays what it was"""
    lay = cl.layout("ladder", 4)
    sh, perm = cl.shuffle_inside_proposals(lay, 3)
    assert not np.array_equal(perm, np.arange(len(perm)))
    a, b = cl.Csr(lay["edge"], lay["bbox_idx"], lay["N"], lay["P"]), cl.Csr(sh["edge"], sh["bbox_idx"], sh["N"], sh["P"])
    assert torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.dst, b.dst)
    owner = sh["bbox_idx"][sh["edge"][:, 1]]
    assert bool((np.diff(owner) >= 0).all())
