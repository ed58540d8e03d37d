"""Plain-loop references of the integer kernels of csrc/subgraph.hip: predict's device selection (yolat_predict_select),
the sub-batch extraction (yolat_expand_ranges, yolat_subgraph_reindex) and the offset fix-up (yolat_fixup_offsets).
numpy and Python only: loops over images, roots, nodes and edges that append to lists or fill dicts, the way
SparseCADGCN.predict (architecture3cc_rpn_gp_iter2.py:153-328) and train.py:238-258 walk them.  No scans, no chunks, no
device code — tests/test_predict_select_ref_host.py checks these against data.py and oracle_torch.py."""
import numpy as np

TREE_KEYS = ("root_row", "root_range", "child_ptr", "child_row", "child_range", "image_root_ptr")
FLAG_TREE, FLAG_EDGES = 1, 2      # bits of the record's word 1 (include/yolat_hip.h, yolat_predict_select)


def argmax_torch_rule(row):
    """torch's ``row.max(0)[1]``: the first index of the maximum; a NaN counts as the maximum, so the first NaN if the
    row holds one"""
    for k, v in enumerate(row):
        if v != v:
            return k
    arg = 0
    for k, v in enumerate(row):
        if v > row[arg]:
            arg = k
    return arg


def select(logits, K, tree):
    """(total, image_off [B + 1], rows [total]) of arch:259-328: per image its roots in order, then, for the roots whose
    arg-max over the K logits is K - 1 (`has_object`), their children in order.  logits: [P, >= K]."""
    root_row, child_ptr, child_row, image_root_ptr = (tree[k] for k in ("root_row", "child_ptr", "child_row",
                                                                        "image_root_ptr"))
    rows, image_off = [], [0]
    for i in range(len(image_root_ptr) - 1):
        children = []
        for r in range(int(image_root_ptr[i]), int(image_root_ptr[i + 1])):
            rows.append(int(root_row[r]))
            if argmax_torch_rule([float(v) for v in logits[int(root_row[r]), :K]]) == K - 1:
                for c in range(int(child_ptr[r]), int(child_ptr[r + 1])):
                    children.append(int(child_row[c]))
        rows += children
        image_off.append(len(rows))
    return len(rows), np.asarray(image_off, dtype=np.int64), np.asarray(rows, dtype=np.int64)


def proposal_ranges(edge, bbox_idx, P):
    """(seg_ptr [P + 1], eptr [P + 1]): first node of every proposal from the sorted bbox_idx, first edge of every proposal
    from an edge list grouped by the proposal of its second endpoint"""
    seg_ptr, eptr = [0] * (P + 1), [0] * (P + 1)
    for p in range(P + 1):
        seg_ptr[p] = sum(1 for b in bbox_idx if b < p)
        eptr[p] = sum(1 for e in edge if bbox_idx[e[1]] < p)
    return np.asarray(seg_ptr, dtype=np.int64), np.asarray(eptr, dtype=np.int64)


def tree_is_proposals(tree, seg_ptr, eptr, P):
    """the rule of k_predict_validate: every root and child row lies in [0, P) and its (idx_pos, idx_edge) ranges are exactly
    the node and edge range of that proposal"""
    for rows, ranges in ((tree["root_row"], tree["root_range"]), (tree["child_row"], tree["child_range"])):
        for row, rg in zip(rows, np.asarray(ranges).reshape(-1, 4)):
            row = int(row)
            if row < 0 or row >= P:
                return False
            if (int(rg[0]), int(rg[1]), int(rg[2]), int(rg[3])) != (int(seg_ptr[row]), int(seg_ptr[row + 1]),
                                                                    int(eptr[row]), int(eptr[row + 1])):
                return False
    return True


def edges_are_local(edge, bbox_idx):
    """every edge stays inside one proposal and the list is grouped by proposal (non-decreasing along the list)"""
    prev = -1
    for a, b in edge:
        pa, pb = int(bbox_idx[int(a)]), int(bbox_idx[int(b)])
        if pa != pb or pb < prev:
            return False
        prev = pb
    return True


def validity_flag(case):
    """word 1 of the record for a case of make_case (possibly doctored): FLAG_TREE | FLAG_EDGES as they apply.  The
    proposals' own ranges come from the case as it was built (seg_ptr, eptr), so only a grouped, local edge list may
    have been doctored together with the tree."""
    local = edges_are_local(case["edge"], case["bbox_idx"])
    flag = 0 if local else FLAG_EDGES
    if not tree_is_proposals(case, case["seg_ptr"], case["eptr"], case["P"]):
        flag |= FLAG_TREE
    return flag


def make_case(child_counts, image_roots, nodes_per_proposal, seed):
    """A grouped graph and its flattened tree, built directly as arrays.  Proposals are consecutive: root r is followed
    by its child_counts[r] children; image i owns image_roots[i] roots (0 allowed).  nodes_per_proposal = (lo, hi).
    bbox_idx is sorted; every proposal has 0..2 edges between its own nodes, appended proposal by proposal."""
    rng = np.random.default_rng(seed)
    child_counts = [int(c) for c in child_counts]
    R, Ctot, B = len(child_counts), sum(child_counts), len(image_roots)
    assert sum(int(v) for v in image_roots) == R
    P = R + Ctot
    lo, hi = nodes_per_proposal
    n_p = rng.integers(lo, hi + 1, size=P)
    e_p = rng.integers(0, 3, size=P)
    seg_ptr = np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64)
    eptr = np.concatenate([[0], np.cumsum(e_p)]).astype(np.int64)
    bbox_idx = np.repeat(np.arange(P, dtype=np.int64), n_p)
    owner = np.repeat(np.arange(P, dtype=np.int64), e_p)
    ends = rng.integers(0, 1 << 30, size=(len(owner), 2)) % n_p[owner][:, None]
    edge = seg_ptr[owner][:, None] + ends
    root_row, root_range, child_ptr, child_row, child_range = [], [], [0], [], []
    p = 0
    for c in child_counts:
        root_row.append(p)
        root_range.append((seg_ptr[p], seg_ptr[p + 1], eptr[p], eptr[p + 1]))
        for q in range(p + 1, p + 1 + c):
            child_row.append(q)
            child_range.append((seg_ptr[q], seg_ptr[q + 1], eptr[q], eptr[q + 1]))
        child_ptr.append(len(child_row))
        p += 1 + c
    image_root_ptr = [0]
    for v in image_roots:
        image_root_ptr.append(image_root_ptr[-1] + int(v))
    bbox = rng.random((P, 4)).astype(np.float32)
    bbox[:, 2:] = bbox[:, :2] + np.float32(0.05) + bbox[:, 2:] * np.float32(0.2)

    def i32(a, shape):
        return np.asarray(a, dtype=np.int64).astype(np.int32).reshape(shape)
    return {"R": R, "Ctot": Ctot, "B": B, "P": P, "N": len(bbox_idx), "E": len(edge),
            "root_row": i32(root_row, (R,)), "root_range": i32(root_range, (R, 4)), "child_ptr": i32(child_ptr, (R + 1,)),
            "child_row": i32(child_row, (Ctot,)), "child_range": i32(child_range, (Ctot, 4)),
            "image_root_ptr": i32(image_root_ptr, (B + 1,)),
            "edge": np.asarray(edge, dtype=np.int64).reshape(-1, 2), "bbox_idx": np.asarray(bbox_idx, dtype=np.int64),
            "seg_ptr": np.asarray(seg_ptr, dtype=np.int64), "eptr": np.asarray(eptr, dtype=np.int64), "bbox": bbox}


# ---------------------------------------------------------------------------------------------
# sub-batch extraction (arch:153-242)
# ---------------------------------------------------------------------------------------------
def expand(starts, prefix, total):
    """the concatenation of range(starts[j], starts[j] + prefix[j + 1] - prefix[j]) (`slice_pos += list(range(...))`)"""
    out = []
    for j in range(len(starts)):
        out += list(range(int(starts[j]), int(starts[j]) + int(prefix[j + 1]) - int(prefix[j])))
    assert len(out) == int(total) == int(prefix[len(starts)])
    return np.asarray(out, dtype=np.int64)


def reindex(node_ids, N, edge, edge_ids, bbox_idx):
    """`build_data` of arch:166-242 -> (edge_out [m, 2], bbox_idx_out [n], missing).  o2n is the reference's dict (a later
    duplicate wins), the edges go through it one by one — a missing key (an endpoint outside the subset, negative or
    >= N) gives -1 and sets `missing`, where the reference raises KeyError — and bbox_idx is renumbered by run length."""
    o2n = {}
    for new_i, old_i in enumerate(node_ids):
        assert 0 <= int(old_i) < N
        o2n[int(old_i)] = new_i
    edge_out, missing = [], False
    for q in edge_ids:
        pair = []
        for v in edge[int(q)]:
            if int(v) in o2n:
                pair.append(o2n[int(v)])
            else:
                pair.append(-1)
                missing = True
        edge_out.append(pair)
    new_idx, count = [], 0
    for i in range(len(node_ids)):
        if i > 0 and bbox_idx[int(node_ids[i])] != bbox_idx[int(node_ids[i - 1])]:
            count += 1
        new_idx.append(count)
    return (np.asarray(edge_out, dtype=np.int64).reshape(-1, 2), np.asarray(new_idx, dtype=np.int64), missing)


def subgraph(node_starts, node_prefix, edge_starts, edge_prefix, N, edge, bbox_idx):
    """expand + reindex: the sub-batch of the node and edge ranges -> (node_ids, edge_ids, edge_out, bbox_idx_out, missing)"""
    node_ids = expand(node_starts, node_prefix, node_prefix[len(node_starts)])
    edge_ids = expand(edge_starts, edge_prefix, edge_prefix[len(edge_starts)])
    return (node_ids, edge_ids) + reindex(node_ids, N, edge, edge_ids, bbox_idx)


def fixup(edge, edge_ptr, bbox_idx, node_ptr, node_off, prop_off):
    """train.py:238-258: per image the sliced in-place adds, on copies"""
    edge, bbox_idx = np.array(edge, dtype=np.int64), np.array(bbox_idx, dtype=np.int64)
    for i in range(len(node_off)):
        edge[int(edge_ptr[i]):int(edge_ptr[i + 1])] += int(node_off[i])
        bbox_idx[int(node_ptr[i]):int(node_ptr[i + 1])] += int(prop_off[i])
    return edge, bbox_idx
