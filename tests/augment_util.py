"""Shared by tests/golden/make_golden_augment.py and the augmentation tests: the synthetic inputs of
tests/golden/augment.npz (seeded, float64 values exactly representable in fp32), items built from them, and the numerics
contract of the augmentation against the reference's float64 outputs."""
import numpy as np

SEEDS = (3, 11, 2024)
# nodes per proposal.  one-node proposals, proposals of more than 64 nodes, every proposal at least one node
CASES = {
    "mixed": dict(sizes=(1, 5, 70, 12, 1, 30, 4, 40), n_gt=5, seed=101),
    "typical": dict(sizes=None, P=24, lo=4, hi=40, n_gt=9, seed=102),
    "long": dict(sizes=(65, 2, 130, 1), n_gt=2, seed=103),
}
# per-item shapes of the cfg-3 / cfg-4 batches (data.config): proposals, nodes lo..hi, items per batch
TIMING_SHAPES = {"cfg3": (2000, 4, 40, 4), "cfg4": (300, 4, 24, 32)}


def _f32_exact(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _inputs(sizes, n_gt, rng):
    sizes = np.asarray(sizes, dtype=np.int64)
    P, N = len(sizes), int(sizes.sum())
    pos = _f32_exact(rng.random((N, 2)))
    bbox_idx = np.repeat(np.arange(P), sizes).astype(np.int64)

    def boxes(n):
        lo = rng.random((n, 2)) * 0.8
        return _f32_exact(np.concatenate([lo, lo + 0.02 + rng.random((n, 2)) * 0.18], 1))
    return {"pos": pos, "bbox_idx": bbox_idx, "bbox": boxes(P), "gt_bbox": boxes(n_gt), "bbox_targets": boxes(P)}


def case_inputs(name):
    kw = CASES[name]
    rng = np.random.default_rng(kw["seed"])
    sizes = kw["sizes"] if kw["sizes"] is not None else rng.integers(kw["lo"], kw["hi"] + 1, size=kw["P"])
    return _inputs(sizes, kw["n_gt"], rng)


def inputs_of_sizes(sizes, seed, n_gt=3):
    return _inputs(sizes, n_gt, np.random.default_rng(seed))


def synth_inputs(P, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return _inputs(rng.integers(lo, hi + 1, size=P), 12, rng)


def item_from_inputs(inp, data_cls, C=5, cols=(3, 4), seed=0):
    """A dataset item around the fixture's inputs: x = [0 .. pos ..] fp32 [N, C], a ring of edges inside every proposal
    of more than one node, random e_attr / stat_feats / labels (none of them is touched by the augmentation)."""
    import torch
    rng = np.random.default_rng(seed)
    pos = inp["pos"].astype(np.float32)
    N, P = pos.shape[0], inp["bbox"].shape[0]
    x = rng.random((N, C)).astype(np.float32)
    x[:, :3] = 0.0
    x[:, cols[0]], x[:, cols[1]] = pos[:, 0], pos[:, 1]
    bidx = inp["bbox_idx"]
    seg = np.searchsorted(bidx, np.arange(P + 1))
    src, dst = [], []
    for p in range(P):
        n = seg[p + 1] - seg[p]
        if n > 1:
            ids = np.arange(seg[p], seg[p + 1])
            src.append(ids)
            dst.append(np.roll(ids, -1))
    edge = np.stack([np.concatenate(src), np.concatenate(dst)], 1).astype(np.int64)
    d = data_cls(x=torch.from_numpy(x), pos=torch.from_numpy(pos.copy()))
    d.edge = torch.from_numpy(edge)
    d.e_attr = torch.from_numpy((rng.standard_normal((edge.shape[0], 4)) * 0.05).astype(np.float32))
    d.bbox_idx = torch.from_numpy(bidx.copy())
    d.bbox = torch.from_numpy(inp["bbox"].astype(np.float32))
    d.stat_feats = torch.from_numpy(rng.random((P, 13)).astype(np.float32))
    d.labels = torch.from_numpy(rng.integers(0, 17, size=P).astype(np.int64))
    d.gt_bbox = torch.from_numpy(inp["gt_bbox"].astype(np.float32))
    d.bbox_targets = torch.from_numpy(inp["bbox_targets"].astype(np.float32))
    return d


def fixture_case(z, name):
    return {k: z["%s/%s" % (name, k)] for k in ("pos", "bbox_idx", "bbox", "gt_bbox", "bbox_targets")}


class Contract(object):
    """|got - want| <= max(spacing of fp32 at |want|, 1e-14) for every element, want = float32(reference float64); over
    everything that was checked, at most 1e-3 of the elements may differ from `want` in their bits.
    (Two correctly ordered float64 evaluations differ by a few float64 ulps at magnitudes <= 3; one rounding to fp32 then
    gives equal or adjacent values.)"""
    CAP = 1e-3

    def __init__(self):
        self.total = 0
        self.not_identical = 0
        self.worst = 0.0

    def check(self, got, want64, what):
        got = np.ascontiguousarray(got)
        assert got.dtype == np.float32, (what, got.dtype)
        want = np.asarray(want64, dtype=np.float64).astype(np.float32)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bound = np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-14)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        self.total += want.size
        self.not_identical += int((got.view(np.uint32) != want.view(np.uint32)).sum())
        if err.size:
            self.worst = max(self.worst, float((err / bound).max()))
        print("augment contract %-28s n=%6d  max err/bound=%.3g  not bit-identical so far=%d of %d"
              % (what, want.size, float((err / bound).max()) if err.size else 0.0, self.not_identical, self.total))
        assert np.all(err <= bound), "%s: %d elements outside the bound, worst err/bound %.3g" % (
            what, int((err > bound).sum()), float((err / bound).max()))

    def finish(self):
        share = self.not_identical / max(self.total, 1)
        print("augment contract: %d of %d elements not bit-identical (share %.3g, cap %.3g)"
              % (self.not_identical, self.total, share, self.CAP))
        assert self.total > 0
        assert share <= self.CAP, "share of elements not bit-identical to the reference %.3g > %.3g" % (share, self.CAP)
