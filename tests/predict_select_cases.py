"""The case lists of the device-selection and sub-graph tests, shared by tests/test_predict_select_ref_host.py (which shows
that every case list tells a correct scan from the usual wrong ones) and the GPU tests of the kernels themselves.  A case
is arrays only: a tree and a graph from predict_select_ref.make_case, and synthetic logits.  numpy only."""
import numpy as np

import predict_select_ref as ref

NAN, INF = float("nan"), float("inf")
CHUNK = 1024        # roots per step of k_predict_select
BLOCK = 4096        # elements per workgroup of k_scan_local


class SelectCase(object):
    def __init__(self, name, case, logits, K):
        self.name, self.case, self.logits, self.K = name, case, logits, K
        self._want = None

    def want(self):
        """(total, image_off, rows) of the plain-loop reference, computed once"""
        if self._want is None:
            self._want = ref.select(self.logits, self.K, self.case)
        return self._want

    def __repr__(self):
        return self.name


def logits_for(case, K, selected, seed):
    """fp32 logits [P, K]: random in [-1, 1), column K - 1 of root r at +2 when selected[r] else at -2 (K = 1: every root
    is selected whatever the row holds)"""
    rng = np.random.default_rng(seed)
    z = (rng.random((case["P"], K)) * 2.0 - 1.0).astype(np.float32)
    rows = case["root_row"].astype(np.int64)
    z[rows, K - 1] = np.where(np.asarray(selected, dtype=bool), np.float32(2.0), np.float32(-2.0))
    return z


def _split(R, B):
    """R roots over B images, as even as it goes"""
    return [R // B + (1 if i < R % B else 0) for i in range(B)]


def _nine_images(R):
    """B = 9: no roots in the first, a middle and the last image; one image boundary at root 1023 and one at root 1024"""
    assert R > 1024
    mid = (1024 + R + 1) // 2
    ptr = [0, 0, 400, 1023, 1024, 1024, mid, max(mid, R - 7), R, R]
    return [ptr[i + 1] - ptr[i] for i in range(9)]


def _counts(R, seed, values=(0, 1, 2, 5)):
    return np.random.default_rng(seed).choice(np.asarray(values), size=R)


ARGMAX_TABLE = {
    5: [[0.0, 2.0, 1.0, 0.0, 2.0],          # a tie of K - 1 with an earlier column: the earlier one
        [2.0, 0.0, 0.0, 0.0, 2.0],          # ... with column 0
        [2.0, 0.0, 2.0, 0.0, 1.0],          # column 0 ties with a later column: column 0
        [3.0, 3.0, 3.0, 3.0, 3.0],          # all equal
        [1.0, 2.0, 0.0, 1.0, NAN],          # NaN in K - 1 only: the maximum
        [1.0, NAN, 0.0, 1.0, 9.0],          # NaN in an earlier column, the finite maximum at K - 1: the NaN
        [NAN, 1.0, 2.0, 3.0, 9.0],          # NaN in column 0
        [1.0, NAN, 0.0, 1.0, NAN],          # two NaNs: the first
        [-INF, -INF, -INF, -INF, 0.0],      # -inf with 0 at K - 1
        [-INF, -INF, -INF, -INF, -INF],     # all -inf
        [0.0, 1.0, INF, 1.0, INF],          # a tie at +inf
        [0.0, 1.0, 2.0, 3.0, 4.0],          # plain: K - 1
        [-1.0, -2.0, -3.0, -0.5, -0.5]],
    3: [[1.0, 2.0, NAN],                    # NaN at K - 1 behind a larger finite value
        [1.0, NAN, 3.0],                    # NaN before the finite maximum at K - 1
        [2.0, 1.0, 2.0],
        [0.0, 2.0, 2.0],
        [3.0, 3.0, 3.0],
        [NAN, 1.0, 9.0],
        [NAN, NAN, NAN],
        [-INF, -INF, 0.0],
        [-INF, -INF, -INF],
        [0.0, 1.0, 2.0]],
}


def _argmax_case(K):
    table = np.asarray(ARGMAX_TABLE[K], dtype=np.float32)
    R = table.shape[0]
    case = ref.make_case([2] * R, _split(R, 2), (1, 2), 300 + K)
    z = (np.random.default_rng(K).random((case["P"], K)) * 2.0 - 1.0).astype(np.float32)
    z[case["root_row"].astype(np.int64)] = table
    return SelectCase("argmax_table_K%d" % K, case, z, K)


_SELECT = []


def select_cases():
    """every case of tests/test_gpu_predict_select.py's comparison with the reference (built once per process)"""
    if _SELECT:
        return _SELECT
    out = []
    seed = 1000
    # sizes x class counts: child counts from {0, 1, 2, 5}, a random half of the roots selected
    for R in (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3100):
        for K in (1, 2, 17, 32):
            seed += 1
            B = 3 if R >= 3 else 1
            case = ref.make_case(_counts(R, seed), _split(R, B), (1, 2), seed)
            sel = np.random.default_rng(seed + 7).random(R) < 0.5
            out.append(SelectCase("size_R%d_K%d" % (R, K), case, logits_for(case, K, sel, seed), K))
    # selection patterns on both sides of the first and the second chunk edge
    for R in (1025, 2049):
        counts = _counts(R, 50 + R)
        counts[[1023, 1024, R - 1]] = (2, 5, 1)
        big = _counts(R, 60 + R, values=(0, 1))
        big[[500, 1024 if R == 1025 else 1500]] = 300      # one hub in the first chunk, one in the second
        patterns = [
            ("none", counts, np.zeros(R, bool)),
            ("all", counts, np.ones(R, bool)),
            ("every_other", counts, np.arange(R) % 2 == 0),
            ("only_1023", counts, np.arange(R) == 1023),
            ("only_1024", counts, np.arange(R) == 1024),
            ("only_last", counts, np.arange(R) == R - 1),
            ("only_childless", counts, counts == 0),
            ("hubs_300", big, (np.random.default_rng(R).random(R) < 0.5) | (big == 300)),
            ("random", counts, np.random.default_rng(R + 1).random(R) < 0.5),
        ]
        for name, cc, sel in patterns:
            for B in (1, 3):
                seed += 1
                case = ref.make_case(cc, _split(R, B), (1, 2), seed)
                out.append(SelectCase("pattern_%s_R%d_B%d" % (name, R, B), case, logits_for(case, 17, sel, seed), 17))
        for name, cc, sel in (patterns[1], patterns[2], patterns[7], patterns[8]):
            seed += 1
            case = ref.make_case(cc, _nine_images(R), (1, 2), seed)
            out.append(SelectCase("pattern_%s_R%d_B9" % (name, R), case, logits_for(case, 17, sel, seed), 17))
    out += [_argmax_case(5), _argmax_case(3)]
    _SELECT.extend(out)
    return _SELECT


# ---------------------------------------------------------------------------------------------
# yolat_subgraph_reindex
# ---------------------------------------------------------------------------------------------
REINDEX_SIZES = (1, 3, 4095, 4096, 4097, 8192, 12289)
REINDEX_PATTERNS = {
    "all_equal": lambda i, n: np.zeros_like(i),
    "all_different": lambda i, n: i,
    "runs_of_7": lambda i, n: i // 7,
    "block_edges": lambda i, n: (i >= BLOCK).astype(np.int64) + (i >= 2 * BLOCK),          # 4095|4096 and 8191|8192 only
    "thread_wave_edges": lambda i, n: (i >= 4).astype(np.int64) + (i >= 64) + (i >= 256),  # 3|4, 63|64, 255|256
    "a_b_a": lambda i, n: np.where((i * 3) // max(n, 1) == 1, 9, 5),                       # non-monotone
}


class ReindexCase(object):
    """node_ids [n] int32 (distinct unless `duplicates`), N, edge [E, 2] int64 over the subset (unless `bad_edges`),
    edge_ids [m] int32, bbox_idx [N] int64 with bbox_idx[node_ids[i]] = pattern(i)"""
    def __init__(self, name, n_sub, pattern, seed, m_sub=None, duplicates=False, bad_edges=False):
        rng = np.random.default_rng(seed)
        self.name = name
        self.N = N = n_sub + 37
        self.node_ids = rng.permutation(N)[:n_sub].astype(np.int32)
        self.bbox_idx = rng.integers(100, 200, size=N).astype(np.int64)
        self.bbox_idx[self.node_ids.astype(np.int64)] = REINDEX_PATTERNS[pattern](np.arange(n_sub, dtype=np.int64), n_sub)
        if duplicates and n_sub >= 3:      # positions that name a node a second time: the later position is its new id
            k = max(1, n_sub // 5)
            dst, src = rng.integers(0, n_sub, size=k), rng.integers(0, n_sub, size=k)
            self.node_ids[dst] = self.node_ids[src]
        E = 0 if n_sub == 0 else max(4, n_sub // 2)
        if n_sub:
            self.edge = self.node_ids.astype(np.int64)[rng.integers(0, n_sub, size=(E, 2))]
        else:
            self.edge = np.zeros((0, 2), dtype=np.int64)
        self.clean = not bad_edges
        if bad_edges:
            inside = set(int(v) for v in self.node_ids)
            outside = [v for v in range(N) if v not in inside]
            self.edge[0, 1] = outside[0]           # a node of the batch that is not in the subset
            self.edge[1, 0] = -1
            self.edge[2, 1] = N
            self.edge[3] = (-5, N + 1000)
        m = (E + 3 if E else 0) if m_sub is None else m_sub
        self.edge_ids = (rng.integers(0, E, size=m) if E else np.zeros(0, dtype=np.int64)).astype(np.int32)
        if bad_edges:
            self.edge_ids[:4] = (0, 1, 2, 3)
        self._want = None

    def want(self):
        if self._want is None:
            self._want = ref.reindex(self.node_ids, self.N, self.edge, self.edge_ids, self.bbox_idx)
        return self._want

    def __repr__(self):
        return self.name


_REINDEX = []


def reindex_cases():
    if _REINDEX:
        return _REINDEX
    out, seed = [], 7000
    for n in REINDEX_SIZES:
        for pat in REINDEX_PATTERNS:
            seed += 1
            out.append(ReindexCase("n%d_%s" % (n, pat), n, pat, seed))
    for n in (3, 4097, 12289):
        seed += 1
        out.append(ReindexCase("n%d_duplicates" % n, n, "runs_of_7", seed, duplicates=True))
        seed += 1
        out.append(ReindexCase("n%d_bad_edges" % n, n, "all_different", seed, bad_edges=True))
    out.append(ReindexCase("n4097_no_edges", 4097, "runs_of_7", seed + 1, m_sub=0))
    out.append(ReindexCase("n0_no_edges", 0, "all_equal", seed + 2, m_sub=0))
    _REINDEX.extend(out)
    return _REINDEX
