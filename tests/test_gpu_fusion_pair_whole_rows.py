"""GPU test, op level: the eval fusion pair at the smallest N where the grid planner (csrc/fusion_x6.hip fx_plan) hands row
tiles to WHOLE-ROW workgroups.  The other op tests stop at N = 600, where every row tile is split into column groups.

N = 65537, F = 192 plans full = 512 (D = 64, 128-row tiles) or 256 (D = 128, 256-row tiles), groups = 2, ng = 2: rows 0..65535
go to workgroups that walk all three column tiles, row 65536 to a tail row tile split into two column groups, the second with
one tile; the P-row second problem runs in front.  Both entry points (yolat_fusion_pair_eval_x6, _f16x3), ReLU and a leaky
slope, per element against float64 with the helpers and the bars of tests/test_gpu_fusion_f16x3.py.  Proposals of uneven
length; one spans rows 65535..65536, the seam between whole-row and tail workgroups, and one is empty."""
import numpy as np
import pytest
import torch

from test_gpu_fusion_f16x3 import TOL64, _act, _run_pair

pytestmark = pytest.mark.gpu

N, F = 65537, 192
_CASES = {}


def _seg():
    """proposal id per row: uneven runs, id 7 empty, the last proposal = rows N - 2, N - 1"""
    rng = np.random.RandomState(65537)
    cuts = np.sort(rng.choice(np.arange(1, N - 2), size=96, replace=False))
    bounds = np.concatenate([[0], cuts, [N - 2, N]])
    ids = np.arange(len(bounds) - 1)
    ids[ids >= 7] += 1                                           # no row carries id 7
    return np.repeat(ids, np.diff(bounds)).astype(np.int32)


def _case(D):
    """operands and the float64 products of one D, built once and shared by the four runs"""
    if D in _CASES:
        return _CASES[D]
    tg = torch.Generator().manual_seed(65537 + D)
    seg = _seg()
    P = int(seg[-1]) + 1
    assert seg[N - 2] == seg[N - 1] == P - 1 and seg[N - 3] != P - 1 and not (seg == 7).any()
    A, S = torch.randn(N, D, generator=tg), torch.randn(P, D, generator=tg)
    W, Ws = torch.randn(F, D, generator=tg) / D ** 0.5, torch.randn(F, D, generator=tg) / D ** 0.5
    s, ss = torch.rand(F, generator=tg) - 0.25, torch.rand(F, generator=tg) - 0.25
    tfold, tsfold = torch.randn(F, generator=tg) * 0.2, torch.randn(F, generator=tg) * 0.2
    y = A.double() @ (W * s[:, None]).double().t() + tfold.double()
    ys = S.double() @ (Ws * ss[:, None]).double().t() + tsfold.double()
    c = dict(N=N, F=F, D=D, P=P, seg=seg, A=A, S=S, W=W, Ws=Ws, s=s, ss=ss, tfold=tfold, tsfold=tsfold, y=y, ys=ys)
    _CASES[D] = c
    return c


@pytest.mark.parametrize("slope", [None, 0.2])
@pytest.mark.parametrize("emul", ["x6", "f16x3"])
@pytest.mark.parametrize("D", [64, 128])
def test_fusion_pair_whole_row_workgroups_vs_fp64(D, emul, slope):
    c = _case(D)
    want = torch.zeros(c["P"], F, dtype=torch.float64)
    want.index_reduce_(0, torch.from_numpy(c["seg"]).long(), _act(c["y"], slope), "amax", include_self=False)
    want_s = _act(c["ys"], None if slope is None else -slope)
    assert bool((want[7] == 0).all())                            # the empty proposal pools to 0
    pool, Ys = _run_pair(c, slope, emul)
    for name, got, ref in (("pool", pool, want), ("super", Ys, want_s)):
        e64 = float((got.double() - ref).abs().max()) / float(ref.abs().max())
        print("%s D=%d %s slope=%s: vs fp64 %.2e of the output scale" % (name, D, emul, slope, e64))
        assert torch.isfinite(got).all(), name
        assert e64 <= TOL64, (name, e64)
