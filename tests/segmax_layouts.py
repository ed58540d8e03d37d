"""Sorted proposal layouts (bbox_idx) aimed at the tiling of the per-proposal max kernels (scatter(max), arch:122).

The training fusion kernels (csrc/fusion_train.hip, fusion_x6.hip, bf16_train.hip) and the eval ones (fusion_x6.hip,
dense.hip) walk rows in 32-row waves, 64-row GEMM / dW blocks and 256-row tiles (the rows kernels, k_fus_da_mfma); the
eval rows kernel reduces the first FX_NP = 32 proposals of a tile in LDS and the rest with direct atomics; k_pool_finish
launches in chunks of 65535 proposals.  Every layout here puts proposal boundaries, empty proposals or long proposals
where one of those tilings changes hands.

layout(name) -> Layout(name, N, P, bbox_idx [N] int64 sorted, sizes [P], edges): `edges` lists the rows at which the
layout claims a new proposal starts (tests/test_segmax_layouts_host.py checks every claim).
"""
from collections import namedtuple

import numpy as np

Layout = namedtuple("Layout", "name N P bbox_idx sizes edges")

FX_NP = 32              # proposals of a 256-row tile reduced in LDS by the eval rows kernel (segmax.hpp)
POOL_CHUNK = 65535      # proposals per k_pool_finish launch (fusion_train.hip)

NAMES = ("one", "straddle", "tiny_then_long", "empty", "aligned", "small_n2", "small_n31", "small_n33", "many", "random")


def _from_sizes(name, sizes, edges=()):
    sizes = np.asarray(sizes, dtype=np.int64)
    bb = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    return Layout(name, int(sizes.sum()), len(sizes), bb, sizes, tuple(int(e) for e in edges))


def _from_starts(name, starts, N, edges=()):
    """proposals starting at the given rows (0 first), the last one running to N"""
    bounds = list(starts) + [N]
    return _from_sizes(name, np.diff(bounds), edges)


def layout(name):
    if name == "one":
        # P = 1 over four 256-row tiles: the middle tiles are first-shared AND last-shared for the same proposal
        return _from_sizes(name, [3 * 256 + 40])
    if name == "straddle":
        # boundaries on both sides of the 32-, 64- and 256-row edges, a proposal of 600 rows (> 512) across two 256-row
        # edges, then the 1024 edge
        starts = [0, 31, 32, 33, 63, 64, 65, 255, 256, 257, 857, 900, 1023, 1024, 1025]
        return _from_starts(name, starts, 1100, edges=starts[1:])
    if name == "tiny_then_long":
        # tile 0: a 100-row proposal, 60 proposals of 1-2 rows (62 proposals in the tile: beyond FX_NP), then a proposal
        # that runs from row 190 into tile 1; tile 1 ends with 40 single-row proposals running into tile 2
        sizes = [100] + [1, 2] * 30 + [300] + [1] * 40 + [150]
        return _from_sizes(name, sizes, edges=(100, 190, 490))
    if name == "empty":
        # empty proposals at id 0, four in a row in the middle, and at id P - 1
        sizes = [0, 40, 3, 0, 0, 0, 0, 70, 1, 200, 0]
        return _from_sizes(name, sizes, edges=(40, 43, 113, 114))
    if name == "aligned":
        # 16 proposals of exactly 32 rows, then 8 of exactly 64 rows: every boundary on a wave / block edge
        sizes = [32] * 16 + [64] * 8
        return _from_sizes(name, sizes, edges=tuple(range(32, 512, 32)) + tuple(range(512, 1024, 64)))
    if name == "small_n2":
        return _from_sizes(name, [2])
    if name == "small_n31":
        return _from_sizes(name, [10, 0, 21], edges=(10,))
    if name == "small_n33":
        return _from_sizes(name, [1, 31, 1], edges=(1, 32))
    if name == "many":
        # more proposals than one k_pool_finish launch takes, one row each
        P = POOL_CHUNK + 300
        return _from_sizes(name, np.ones(P, dtype=np.int64), edges=(POOL_CHUNK,))
    if name == "random":
        # the multinomial layout of test_gpu_ops.py's fusion test (one empty proposal)
        Nn, P = 5000, 300
        rng = np.random.default_rng(Nn)
        n_p = rng.multinomial(Nn - P + 1, np.ones(P - 1) / (P - 1)) + 1
        n_p = np.concatenate([n_p[:3], [0], n_p[3:]])
        n_p[-1] += Nn - n_p.sum()
        return _from_sizes(name, n_p)
    raise KeyError(name)


def starts(lay):
    """first row of every proposal (an empty proposal: the first row of the next one)"""
    return np.concatenate([[0], np.cumsum(lay.sizes)[:-1]])


def tie_proposals(lay):
    """Proposals to fill with bit-identical copies of one row: the first one that spans a multiple of 64 that is not a
    multiple of 256, and the first one that spans a multiple of 256 (neither the whole batch).  Every column of such a
    proposal ties across a GEMM block edge or a 256-row tile edge."""
    st = starts(lay)
    out = []
    for want256 in (False, True):
        for p in range(lay.P):
            lo, hi = int(st[p]), int(st[p] + lay.sizes[p])      # rows [lo, hi)
            if hi - lo < 2 or hi - lo == lay.N:
                continue
            e = (lo // 64 + 1) * 64                              # first 64-row edge after lo
            hit = [x for x in range(e, hi, 64) if (x % 256 == 0) == want256]
            if hit and p not in out:
                out.append(p)
                break
    return out
