"""The proposal layouts of tests/segmax_layouts.py are what they claim to be (no GPU needed)."""
import numpy as np
import pytest

import segmax_layouts as sl

pytestmark = pytest.mark.host


def _tiles_of(lay, rows):
    """proposal ids present in each `rows`-row tile"""
    return [set(lay.bbox_idx[r0:r0 + rows].tolist()) for r0 in range(0, lay.N, rows)]


@pytest.mark.parametrize("name", sl.NAMES)
def test_layout_is_sorted_and_hits_its_edges(name):
    lay = sl.layout(name)
    bb = lay.bbox_idx
    assert bb.dtype == np.int64 and bb.shape == (lay.N,) and lay.N >= 2          # training BatchNorm needs N >= 2
    assert np.all(np.diff(bb) >= 0) and bb.min() >= 0 and bb.max() < lay.P
    assert len(lay.sizes) == lay.P and int(lay.sizes.sum()) == lay.N
    assert np.array_equal(np.bincount(bb, minlength=lay.P), lay.sizes)
    for e in lay.edges:
        assert 0 < e < lay.N and bb[e - 1] != bb[e], (name, e)
    st = sl.starts(lay)
    for p in sl.tie_proposals(lay):
        lo, hi = int(st[p]), int(st[p] + lay.sizes[p])
        assert hi - lo >= 2 and hi - lo < lay.N and any(lo < x < hi for x in range(64, lay.N, 64)), (name, p)

    if name == "one":
        assert lay.P == 1 and lay.N == 3 * 256 + 40
        # a middle 256-row tile: shared with the previous AND the next tile by the one proposal
        assert bb[255] == bb[256] == bb[511] == bb[512]
    elif name == "straddle":
        assert {31, 32, 33, 63, 64, 65, 255, 256, 257} <= set(lay.edges)
        assert lay.sizes.max() > 512
        long_p = int(np.argmax(lay.sizes))
        assert len([x for x in range(256, lay.N, 256) if st[long_p] < x < st[long_p] + lay.sizes[long_p]]) >= 2
    elif name == "tiny_then_long":
        tile0 = sorted(_tiles_of(lay, 256)[0])
        assert len(tile0) > sl.FX_NP
        assert all(lay.sizes[p] <= 2 for p in tile0[1:-1])
        assert bb[255] == bb[256] == tile0[-1]                # the last proposal of tile 0 runs into tile 1
    elif name == "empty":
        s = lay.sizes
        assert s[0] == 0 and s[-1] == 0
        inner = np.flatnonzero(s[1:-1] == 0) + 1
        assert any(inner[i + 1] == inner[i] + 1 for i in range(len(inner) - 1))          # consecutive empties
    elif name == "aligned":
        assert list(lay.sizes) == [32] * 16 + [64] * 8
        assert all(st[p] % lay.sizes[p] == 0 for p in range(lay.P))
    elif name.startswith("small_n"):
        assert lay.N == int(name[len("small_n"):]) and lay.N in (2, 31, 33)
    elif name == "many":
        assert lay.P == sl.POOL_CHUNK + 300 and lay.P > sl.POOL_CHUNK and (lay.sizes == 1).all()
    elif name == "random":
        assert lay.P == 300 and lay.N == 5000 and (lay.sizes == 0).sum() == 1


def test_tie_proposals_cross_a_64_and_a_256_row_edge():
    for name in ("straddle", "tiny_then_long", "empty", "random"):
        lay = sl.layout(name)
        st = sl.starts(lay)
        ties = sl.tie_proposals(lay)
        assert len(ties) == 2, name
        spans = [[x for x in range(64, lay.N, 64) if st[p] < x < st[p] + lay.sizes[p]] for p in ties]
        assert any(x % 256 for x in spans[0]), name
        assert any(x % 256 == 0 for x in spans[1]), name
