"""GPU tests of predict's device selection, yolat_predict_select and yolat_predict_gather (csrc/subgraph.hip), called
directly: hand-built trees (tests/predict_select_ref.make_case — a collated batch cannot have an image without roots) and
synthetic logits against the plain loops of tests/predict_select_ref.py, with array_equal.  No model forward.  The cases
(tests/predict_select_cases.py) put roots, selected children and image boundaries on both sides of the 1024-root chunk of
k_predict_select; tests/test_predict_select_ref_host.py shows that they notice a wrong carry, chunk total, image offset,
row order and arg-max rule.  Conventions: the logits are a column slot of a wider NaN-filled buffer, the record is
followed by 64 guard words that keep their bits (so do the rows behind `total`), every call runs twice with equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import predict_select_cases as pc
import predict_select_ref as ref

pytestmark = pytest.mark.gpu

SENT = -0x21524111          # 0xDEADBEEF as int32
GUARD = 64


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tree(case):
    """the tree arrays in one device buffer -> (yolat_predict_tree, the buffer)"""
    from yolat_vectorgraphicsrecognition_amd._lib import PredictTree
    parts, offs, o = [], {}, 0
    for k in ref.TREE_KEYS:
        a = np.ascontiguousarray(case[k], dtype=np.int32).reshape(-1)
        offs[k] = o
        o += a.size
        parts.append(a)
    buf = _dev(np.concatenate(parts + [np.zeros(1, dtype=np.int32)]))
    t = PredictTree()
    t.R, t.Ctot, t.B = case["R"], case["Ctot"], case["B"]
    for k in ref.TREE_KEYS:
        setattr(t, k, buf.data_ptr() + 4 * offs[k])
    return t, buf


def _logit_slot(z, K):
    """z [P, K] as columns [2, 2 + K) of a NaN-filled [P, K + 5] device buffer -> (buffer, address of the slot, ld)"""
    full = torch.full((z.shape[0], K + 5), float("nan"), dtype=torch.float32, device="cuda")
    full[:, 2:2 + K] = _dev(z)
    return full, full.data_ptr() + 4 * 2, K + 5


def run_select(case, z, K):
    """yolat_predict_select twice on fresh sentinel-filled records -> the record of the first run (numpy int32, guard
    words included); asserts the second run's bits and the workspace guard"""
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    t, tbuf = _tree(case)
    full, zp, ld = _logit_slot(z, K)
    edge, bbox_idx = _dev(case["edge"].astype(np.int64)), _dev(case["bbox_idx"].astype(np.int64))
    N, E, P, B = case["N"], case["E"], case["P"], case["B"]
    words = 4 + B + 1 + case["R"] + case["Ctot"]
    need = int(lib.yolat_predict_select_workspace_bytes(N, P, case["R"]))
    assert need > 0
    records = []
    for _ in range(2):
        out = torch.full((words + GUARD,), SENT, dtype=torch.int32, device="cuda")
        ws = torch.full((need + 512,), 0xAB, dtype=torch.uint8, device="cuda")
        check(lib.yolat_predict_select(zp, ld, P, K, edge.data_ptr() if E > 0 else None, 2, 1, bbox_idx.data_ptr(), N, E,
                                       ctypes.byref(t), out.data_ptr(), ws.data_ptr(), need, yv.ops._stream()),
              "yolat_predict_select")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xAB).all()), "the workspace guard was written"
        records.append(out.cpu().numpy())
    assert records[0].tobytes() == records[1].tobytes(), "two runs differ"
    assert bool(torch.isnan(full[:, :2]).all()) and bool(torch.isnan(full[:, 2 + K:]).all())
    return records[0]


def check_record(out, case, want, name):
    total, image_off, rows = want
    B = case["B"]
    head = 4 + B + 1
    got_total = int(out[0])
    got_rows = out[head:head + max(0, min(got_total, case["R"] + case["Ctot"]))]
    msg = "%s: got total %d flag %d image_off %s, expected total %d flag 0 image_off %s" % (
        name, got_total, int(out[1]), out[4:head].tolist(), total, image_off.tolist())
    assert got_total == total and int(out[1]) == 0, msg
    assert int(out[2]) == 0 and int(out[3]) == 0, msg
    assert np.array_equal(out[4:head], image_off), msg
    if not np.array_equal(got_rows, rows):
        at = int(np.flatnonzero(got_rows != rows)[0])
        raise AssertionError("%s: rows differ first at %d: got %s, expected %s" % (name, at, got_rows[at:at + 8].tolist(),
                                                                                   rows[at:at + 8].tolist()))
    assert np.all(out[head + total:] == SENT), "%s: words behind the last row were written" % name


SIZE_GROUPS = ["size_R%d_" % R for R in (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3100)]
PATTERN_GROUPS = ["pattern_%s_R%d_" % (p, R) for R in (1025, 2049)
                  for p in ("none", "all", "every_other", "only_1023", "only_1024", "only_last", "only_childless", "hubs_300",
                            "random")]


@pytest.mark.parametrize("group", SIZE_GROUPS + PATTERN_GROUPS)
def test_record_equals_the_plain_loop_reference(group):
    cases = [sc for sc in pc.select_cases() if sc.name.startswith(group)]
    assert len(cases) >= 2
    for sc in cases:
        check_record(run_select(sc.case, sc.logits, sc.K), sc.case, sc.want(), sc.name)


def test_every_select_case_belongs_to_a_group():
    names = [sc.name for sc in pc.select_cases()]
    groups = SIZE_GROUPS + PATTERN_GROUPS + ["argmax_table_K"]
    assert all(sum(n.startswith(g) for g in groups) == 1 for n in names)


@pytest.mark.parametrize("K", [5, 3])
def test_arg_max_is_the_first_maximum_and_a_nan_is_the_maximum(K):
    """has_object of the one-submission path = `pred_cls.max(1)[1] == K - 1` of the two-pass path and of the reference: the
    first index of the row maximum, a NaN counting as the maximum (the rule k_eval_rows states).
    k_predict_select used to take `if (v > best)`, which skips NaNs.  Measured on the MI355X with that kernel, children
    selected (got / expected): K = 3: [1, 2, NaN] no / yes, [1, NaN, 3] yes / no; K = 5: [1, 2, 0, 1, NaN] no / yes,
    [1, NaN, 0, 1, 9] yes / no; every other row of the table agreed (the totals too — 16 and 19 rows — since one root lost
    two children where another gained two).  Since then both kernels call yl_argmax_row (csrc/sel_record.hpp)."""
    sc = [c for c in pc.select_cases() if c.name == "argmax_table_K%d" % K][0]
    table = np.asarray(pc.ARGMAX_TABLE[K], dtype=np.float32)
    rule = [ref.argmax_torch_rule([float(v) for v in row]) for row in table]
    two_pass = _dev(table).max(1)[1].cpu().tolist()                  # the two-pass rule, on the device
    assert two_pass == rule
    roots = sc.case["root_row"].astype(np.int64)
    assert sc.logits[roots].tobytes() == table.tobytes() and np.all(np.diff(sc.case["child_ptr"]) == 2)
    out = run_select(sc.case, sc.logits, sc.K)
    # which roots brought their children: read off the record, per image
    B, R = sc.case["B"], sc.case["R"]
    head = 4 + B + 1
    got_rows = out[head:head + max(0, int(out[0]))].tolist()
    got_has = [int(sc.case["child_row"][sc.case["child_ptr"][r]]) in got_rows for r in range(R)]
    want_has = [a == K - 1 for a in rule]
    print("K = %d: has_object got %s expected %s; total got %d expected %d; image_off got %s expected %s"
          % (K, got_has, want_has, int(out[0]), sc.want()[0], out[4:head].tolist(), sc.want()[1].tolist()))
    assert got_has == want_has, [(table[r].tolist(), got_has[r], want_has[r]) for r in range(R) if got_has[r] != want_has[r]]
    check_record(out, sc.case, sc.want(), sc.name)


# ---------------------------------------------------------------------------------------------
# the validity word
# ---------------------------------------------------------------------------------------------
def _validity_case():
    case = ref.make_case(np.random.default_rng(9).choice([0, 1, 2], size=600), [200, 0, 400], (1, 3), 77)
    assert case["R"] > 256 + 44 and case["E"] > 10
    return case, pc.logits_for(case, 4, np.arange(600) % 3 == 0, 5)


def _doctor(case, key, at, value=None, delta=0):
    bad = dict(case)
    bad[key] = case[key].copy()
    bad[key][at] = case[key][at] + delta if value is None else value
    return bad


def test_validity_word_is_zero_for_a_clean_tree_and_names_what_is_wrong():
    case, z = _validity_case()
    out = run_select(case, z, 4)
    check_record(out, case, ref.select(z, 4, case), "clean")
    P = case["P"]
    tree_cases = {
        "root_range_at_root_0": _doctor(case, "root_range", (0, 1), delta=1),
        "root_range_at_root_300": _doctor(case, "root_range", (300, 2), delta=1),      # second block of k_predict_validate
        "root_range_start_at_root_599": _doctor(case, "root_range", (599, 0), delta=-1),
        "child_range": _doctor(case, "child_range", (case["Ctot"] - 1, 3), delta=1),
        "root_row_equal_to_P": _doctor(case, "root_row", 5, value=P),
        "root_row_minus_one": _doctor(case, "root_row", 5, value=-1),
        "child_row_equal_to_P": _doctor(case, "child_row", 0, value=P),
    }
    for name, bad in tree_cases.items():
        assert ref.validity_flag(bad) == ref.FLAG_TREE, name
        out = run_select(bad, z, 4)
        assert int(out[1]) == ref.FLAG_TREE, (name, int(out[1]))
    # an edge that crosses into another proposal: its second endpoint stays, so every proposal keeps its edge range
    e = int(case["E"] // 2)
    owner = int(case["bbox_idx"][case["edge"][e, 1]])
    other = int(case["seg_ptr"][owner + 1 if owner + 1 < P else owner - 1])
    crossing = _doctor(case, "edge", (e, 0), value=other)
    assert ref.validity_flag(crossing) == ref.FLAG_EDGES
    assert int(run_select(crossing, z, 4)[1]) == ref.FLAG_EDGES
    # a list that is not grouped by proposal: the first and the last edge change places
    ungrouped = dict(case, edge=case["edge"].copy())
    ungrouped["edge"][[0, -1]] = case["edge"][[-1, 0]]
    assert case["bbox_idx"][case["edge"][0, 1]] != case["bbox_idx"][case["edge"][-1, 1]]
    assert ref.validity_flag(ungrouped) & ref.FLAG_EDGES
    assert int(run_select(ungrouped, z, 4)[1]) & ref.FLAG_EDGES


# ---------------------------------------------------------------------------------------------
# yolat_predict_gather on the selected rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17])
@pytest.mark.parametrize("total", [0, 1, 255, 256, 257])
def test_gather_is_bit_equal_to_the_logits_rows_and_the_two_pass_box_steps(total, K):
    yv = _yv()
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    # `total` rows: R roots of which the first brings 10 children (total > 10), else the roots alone
    kids = 10 if total > 10 else 0
    R = max(total - kids, 1)
    counts = np.zeros(R, dtype=np.int64)
    counts[0] = kids
    if K > 1 and R > 1:
        counts[R - 1] = 3                                            # children that are not selected (K = 1 selects all)
    case = ref.make_case(counts, pc._split(R, min(R, 2)), (1, 2), 500 + total)
    z = pc.logits_for(case, K, np.arange(R) == 0, 9)
    z[case["P"] - 1, 0] = np.float32("nan")                          # bits, not values, are compared
    z[0, 0] = np.float32(-0.0)
    want_total, _, want_rows = ref.select(z, K, case)
    if total == 0:
        want_total, want_rows = 0, want_rows[:0]
    assert want_total == total
    out = _dev(run_select(case, z, K))
    full, zp, ld = _logit_slot(z, K)
    bbox = _dev(case["bbox"])
    rows_ptr = out.data_ptr() + 4 * (4 + case["B"] + 1)
    got = []
    for _ in range(2):
        cls = torch.full((total * K + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda")
        box = torch.full((total * 4 + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda")
        check(lib.yolat_predict_gather(zp, ld, case["P"], K, bbox.data_ptr(), rows_ptr, total, cls.data_ptr() + 4 * GUARD,
                                       box.data_ptr() + 4 * GUARD, yv.ops._stream()), "yolat_predict_gather")
        torch.cuda.synchronize()
        got.append((cls.cpu().numpy(), box.cpu().numpy()))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    cls, box = got[0]
    for a in (cls, box):
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT)
    assert cls[GUARD:-GUARD].tobytes() == np.ascontiguousarray(z[want_rows, :K]).tobytes()
    # architecture.py, _predict_two_pass: the same fp32 steps by torch on the device, on the same rows
    pred_bbox = bbox[_dev(want_rows)]
    w = (pred_bbox[:, 2] - pred_bbox[:, 0]) * 1.05
    h = (pred_bbox[:, 3] - pred_bbox[:, 1]) * 1.05
    cx = (pred_bbox[:, 2] + pred_bbox[:, 0]) / 2
    cy = (pred_bbox[:, 3] + pred_bbox[:, 1]) / 2
    want_box = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=1)
    assert box[GUARD:-GUARD].tobytes() == want_box.contiguous().cpu().numpy().tobytes()
