"""GPU tests of the extraction kernels of csrc/subgraph.hip called directly — yolat_expand_ranges, yolat_subgraph_reindex,
yolat_gather_rows_bytes, yolat_fixup_offsets — against the plain loops of tests/predict_select_ref.py with array_equal, at
the sizes where the block-local scan of the renumbering (4096 elements per workgroup, 4 per thread, 16 waves) and the
256-thread launches change blocks.  Every output is a slot of a sentinel-filled buffer whose other words keep their bits,
and every call runs twice with equal bits.  The reindex cases are tests/predict_select_cases.reindex_cases(), which
tests/test_predict_select_ref_host.py shows to notice dropped or misplaced block totals."""
import numpy as np
import pytest
import torch

import predict_select_cases as pc
import predict_select_ref as ref

pytestmark = pytest.mark.gpu

SENT = -0x21524111          # 0xDEADBEEF as int32
SENT64 = -0x2152411021524111
GUARD = 64


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _lib():
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    return lib, check


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slot(n, dtype, sent):
    """a sentinel-filled device buffer of GUARD + n + GUARD elements -> (buffer, address of element GUARD)"""
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _guards_intact(buf, sent):
    a = buf.cpu().numpy()
    return bool(np.all(a[:GUARD] == sent) and np.all(a[-GUARD:] == sent))


def _twice(fn):
    """fn() -> tuple of numpy arrays, run twice: equal bits"""
    a, b = fn(), fn()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two runs differ"
    return a


# ---------------------------------------------------------------------------------------------
# yolat_expand_ranges
# ---------------------------------------------------------------------------------------------
def _lengths(S, total, rng):
    """S range lengths that sum to `total`, zero at the first, the last and three middle ranges where S allows it"""
    if S == 1:
        return [np.array([total])]
    if S == 2:
        return [np.array([total // 3, total - total // 3]), np.array([0, total]), np.array([total, 0])]
    cut = np.sort(rng.integers(0, total + 1, size=S - 1))
    lens = np.diff(np.concatenate([[0], cut, [total]]))
    for z in (0, S - 1, S // 2, S // 2 + 1, S // 2 + 2):
        lens[S // 3] += lens[z]
        lens[z] = 0
    return [lens]


@pytest.mark.parametrize("S", [1, 2, 1000])
def test_expand_ranges(S):
    yv = _yv()
    lib, check = _lib()
    rng = np.random.default_rng(S)
    for total in (0, 1, 255, 256, 257, 5000):
        for lens in _lengths(S, total, rng):
            assert lens.sum() == total and len(lens) == S and lens.min() >= 0
            starts = rng.integers(0, 1 << 20, size=S).astype(np.int32)
            prefix = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            want = ref.expand(starts, prefix, total)
            st, pf = _dev(starts), _dev(prefix)

            def run():
                out, p = _slot(total, torch.int32, SENT)
                check(lib.yolat_expand_ranges(st.data_ptr(), pf.data_ptr(), S, total, p, yv.ops._stream()),
                      "yolat_expand_ranges")
                torch.cuda.synchronize()
                assert _guards_intact(out, SENT)
                return (out.cpu().numpy()[GUARD:GUARD + total],)
            got, = _twice(run)
            assert np.array_equal(got, want), (S, total, lens[:4])


# ---------------------------------------------------------------------------------------------
# yolat_subgraph_reindex
# ---------------------------------------------------------------------------------------------
def run_reindex(rc, transposed):
    yv = _yv()
    lib, check = _lib()
    n, m, N = len(rc.node_ids), len(rc.edge_ids), rc.N
    node_ids, edge_ids, bbox_idx = _dev(rc.node_ids), _dev(rc.edge_ids), _dev(rc.bbox_idx)
    if transposed:          # the [E, 2] view of a [2, E] tensor: stride_e = 1, stride_c = E
        edge = _dev(np.ascontiguousarray(rc.edge.T)).t()
    else:
        edge = _dev(rc.edge)
    E = rc.edge.shape[0]
    assert edge.shape == (E, 2) and (E == 0 or (edge.stride(0), edge.stride(1)) == ((1, E) if transposed else (2, 1)))
    work_elems = int(lib.yolat_subgraph_work_elems(N, n))

    def run():
        edge_out, pe = _slot(2 * m, torch.int64, SENT64)
        bidx_out, pb = _slot(n, torch.int64, SENT64)
        status, ps = _slot(1, torch.int32, SENT)
        status[GUARD] = 0
        work, pw = _slot(work_elems, torch.int32, SENT)
        check(lib.yolat_subgraph_reindex(node_ids.data_ptr(), n, N, edge.data_ptr() if m else None, edge.stride(0) if E else 2,
                                         edge.stride(1) if E else 1, edge_ids.data_ptr() if m else None, m, bbox_idx.data_ptr(),
                                         pe, pb, pw, ps, yv.ops._stream()), "yolat_subgraph_reindex")
        torch.cuda.synchronize()
        for buf, s in ((edge_out, SENT64), (bidx_out, SENT64), (status, SENT), (work, SENT)):
            assert _guards_intact(buf, s)
        return (edge_out.cpu().numpy()[GUARD:GUARD + 2 * m].reshape(m, 2), bidx_out.cpu().numpy()[GUARD:GUARD + n],
                status.cpu().numpy()[GUARD:GUARD + 1])
    return _twice(run)


@pytest.mark.parametrize("n_sub", pc.REINDEX_SIZES + (0,))
def test_subgraph_reindex(n_sub):
    yv = _yv()
    cases = [rc for rc in pc.reindex_cases() if len(rc.node_ids) == n_sub]
    assert cases
    for rc in cases:
        want_edge, want_bidx, missing = rc.want()
        for transposed in (False, True):
            edge_out, bidx_out, status = run_reindex(rc, transposed)
            assert np.array_equal(bidx_out, want_bidx), rc.name
            assert np.array_equal(edge_out, want_edge), rc.name
            assert int(status[0]) == (yv.ops.STATUS_EDGE_RANGE if missing else 0), (rc.name, int(status[0]))
        if missing:
            assert int((want_edge < 0).sum()) >= 5 and (want_edge >= 0).any()


# ---------------------------------------------------------------------------------------------
# yolat_gather_rows_bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", [4, 8, 20, 52])
def test_gather_rows_bytes_between_column_slots(row_bytes):
    """source and destination rows are column slices of wider tensors (a row stride on both sides); whatever lies
    outside the destination slot keeps its bits"""
    yv = _yv()
    lib, check = _lib()
    rng = np.random.default_rng(row_bytes)
    words = row_bytes // 4
    n_src, w_src, c_src = 300, words + 5, 2
    w_dst, c_dst = words + 3, 1
    src_h = rng.integers(-(1 << 31), 1 << 31, size=(n_src, w_src)).astype(np.int32)
    src = _dev(src_h)
    for rows in (0, 1, 255, 256, 257, 1000):
        idx_h = rng.integers(0, n_src, size=rows).astype(np.int32)
        if rows > 3:
            idx_h[1] = idx_h[0]                  # repeated indices
            idx_h[-1] = idx_h[0]
        idx = _dev(idx_h) if rows else torch.zeros(1, dtype=torch.int32, device="cuda")

        def run():
            dst = torch.full((rows + 2, w_dst), SENT, dtype=torch.int32, device="cuda")
            check(lib.yolat_gather_rows_bytes(src.data_ptr() + 4 * c_src, 4 * w_src, idx.data_ptr(), rows, row_bytes,
                                              dst.data_ptr() + 4 * (w_dst + c_dst), 4 * w_dst, yv.ops._stream()),
                  "yolat_gather_rows_bytes")
            torch.cuda.synchronize()
            return (dst.cpu().numpy(),)
        got, = _twice(run)
        want = np.full((rows + 2, w_dst), SENT, dtype=np.int32)
        for r in range(rows):
            want[1 + r, c_dst:c_dst + words] = src_h[idx_h[r], c_src:c_src + words]
        assert np.array_equal(got, want), (row_bytes, rows)


def test_gather_rows_bytes_of_an_int64_tensor():
    yv = _yv()
    lib, check = _lib()
    src_h = np.random.default_rng(8).integers(-(1 << 62), 1 << 62, size=(77, 3)).astype(np.int64)
    idx_h = np.random.default_rng(9).integers(0, 77, size=300).astype(np.int32)
    src, idx = _dev(src_h), _dev(idx_h)
    dst, p = _slot(300, torch.int64, SENT64)
    check(lib.yolat_gather_rows_bytes(src.data_ptr() + 8, 24, idx.data_ptr(), 300, 8, p, 8, yv.ops._stream()),
          "yolat_gather_rows_bytes")
    torch.cuda.synchronize()
    assert _guards_intact(dst, SENT64) and np.array_equal(dst.cpu().numpy()[GUARD:-GUARD], src_h[idx_h, 1])


# ---------------------------------------------------------------------------------------------
# yolat_fixup_offsets
# ---------------------------------------------------------------------------------------------
def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


FIXUP_CASES = {
    # name: (edges per image, nodes per image)
    "B1_E_gt_N": ([700], [300]),
    "B1_E_lt_N": ([300], [700]),
    "B1_E_zero": ([0], [300]),
    "B5_E_gt_N": ([200, 0, 257, 0, 300], [100, 50, 0, 7, 143]),        # images without edges, one without nodes
    "B5_E_lt_N": ([100, 50, 0, 7, 143], [200, 0, 257, 0, 300]),
    "B5_E_zero": ([0, 0, 0, 0, 0], [256, 0, 1, 255, 3]),
    "B5_an_image_with_nothing": ([256, 0, 300, 1, 0], [255, 0, 300, 2, 0]),
    "B5_empty_first_image": ([0, 3, 600, 1, 9], [0, 5, 100, 1, 9]),
}


@pytest.mark.parametrize("name", sorted(FIXUP_CASES))
def test_fixup_offsets(name):
    yv = _yv()
    lib, check = _lib()
    e_n, n_n = FIXUP_CASES[name]
    B, E, N = len(e_n), sum(e_n), sum(n_n)
    rng = np.random.default_rng(len(name) + E)
    edge_ptr, node_ptr = _ptr(e_n), _ptr(n_n)
    node_off = rng.integers(0, 1 << 40, size=B).astype(np.int64)       # beyond 32 bits: the adds are 64-bit
    prop_off = rng.integers(0, 1 << 40, size=B).astype(np.int64)
    edge_h = rng.integers(0, 1000, size=(E, 2)).astype(np.int64)
    bidx_h = rng.integers(0, 1000, size=N).astype(np.int64)
    want_edge, want_bidx = ref.fixup(edge_h, edge_ptr, bidx_h, node_ptr, node_off, prop_off)
    ptrs = [_dev(a) for a in (edge_ptr, node_ptr, node_off, prop_off)]

    def run():
        edge, pe = _slot(2 * E, torch.int64, SENT64)
        bidx, pb = _slot(N, torch.int64, SENT64)
        edge[GUARD:GUARD + 2 * E] = _dev(edge_h).reshape(-1)
        bidx[GUARD:GUARD + N] = _dev(bidx_h)
        check(lib.yolat_fixup_offsets(pe if E else None, E, ptrs[0].data_ptr(), pb, N, ptrs[1].data_ptr(), ptrs[2].data_ptr(),
                                      ptrs[3].data_ptr(), B, yv.ops._stream()), "yolat_fixup_offsets")
        torch.cuda.synchronize()
        assert _guards_intact(edge, SENT64) and _guards_intact(bidx, SENT64)
        return edge.cpu().numpy()[GUARD:GUARD + 2 * E].reshape(E, 2), bidx.cpu().numpy()[GUARD:GUARD + N]
    got_edge, got_bidx = _twice(run)
    assert np.array_equal(got_edge, want_edge) and np.array_equal(got_bidx, want_bidx)
    if E:
        assert not np.array_equal(got_edge, edge_h)
