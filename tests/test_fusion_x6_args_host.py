"""CPU test (-m "not gpu") of the argument checks of the bf16x6 / f16x3 rows-kernel ops: the eval fusion pair in its four
exported forms (yolat_fusion_pair_eval_x6[_act], yolat_fusion_pair_eval_f16x3[_act]) and behind a row norm
(yolat_fusion_pair_eval_x6_rn), the weight splits (yolat_split_bf16x3, yolat_split_f16x2, yolat_split_bf16x3_packed), the
skinny classifier Linear (yolat_linear_x6, yolat_linear_x6_pre), the training Linear on the rows kernel
(yolat_linear_fwd_rows_x6) and the node side (yolat_node_uv_eval_x6).  The table pins the return code of every rejected call,
one row per term of every check, and yolat_split_bf16x3_packed_elems as exact numbers, so that code which moves between
files or is folded into one checker cannot move a code.  The addresses are fake: every row returns before a launch (a row
that would launch has no place here), so no GPU is needed.

The _act forms start yolat_pool_init_signed before the checks they share with the ReLU forms: only their own three NULL
checks are pinned.  The x6 and the f16x3 pair differ in one term, P * ldys >= 2^32: f16x3 declines it; the x6 call of that
shape would launch, so only the f16x3 row can stand here."""
import ctypes

import pytest

from yolat_vectorgraphicsrecognition_amd import _lib

INVALID, UNSUPPORTED = -1, -2
A = 0x10000          # 16-byte aligned
A8 = 0x10008         # 8-byte aligned only
E31 = 1 << 31


def edit(base, **kw):
    """the tuple `base` (a call that would launch) with the named positions replaced: edit(base, _3=0, _7=None)"""
    out = list(base)
    for k, v in kw.items():
        out[int(k[1:])] = v
    return tuple(out)


def rows(fn, base, table):
    return [(fn, edit(base, **kw), rc) for kw, rc in table]


def nulls(*positions):
    return [({"_%d" % i: None}, INVALID) for i in positions]


def misaligned(*positions):
    return [({"_%d" % i: A8}, UNSUPPORTED) for i in positions]


# ---- yolat_fusion_pair_eval_x6(A, lda, N, D, Wh, Wm, Wl, tfold, F, node_seg, pool, ldpool, S, lds, P, Wsh, Wsm, Wsl, tsfold,
#                                Ys, ldys, stream)
#      yolat_fusion_pair_eval_f16x3: (Wh, Wl, Wexp) and (Wsh, Wsl, Wsexp) in the places of the three-way splits
PAIR = (A, 64, 10, 64, A, A, A, A, 64, A, A, 64, A, 64, 4, A, A, A, A, A, 64, None)
# ---- the _act forms: slope_f after F, seg_ptr after node_seg, slope_s after tsfold
PAIR_ACT = (A, 64, 10, 64, A, A, A, A, 64, A, A, A, A, 64, A, 64, 4, A, A, A, A, A, A, 64, None)
PAIR_SHARED = [
    (dict(_2=0), INVALID), (dict(_14=0), INVALID), (dict(_8=0), INVALID),
    *nulls(0, 4, 5, 6, 7, 9, 10, 12, 15, 16, 17, 18, 19),
    (dict(_2=E31 - 256), INVALID), (dict(_1=60), INVALID), (dict(_13=60), INVALID), (dict(_11=60), INVALID),
    (dict(_20=60), INVALID),
    (dict(_3=96, _1=96, _13=96), UNSUPPORTED), (dict(_8=32), UNSUPPORTED),
    (dict(_1=66), UNSUPPORTED), (dict(_13=66), UNSUPPORTED),
    *misaligned(0, 12),
    (dict(_14=1 << 26), UNSUPPORTED),                    # P * ldpool = 2^32
]
# ---- yolat_split_bf16x3(W, ldw, rows, cols, row_scale, hi, mid, lo, stream); yolat_split_f16x2: (hi, lo, exps)
SPLIT = (A, 64, 4, 64, None, A, A, A, None)
SPLIT_SHARED = [(dict(_2=0), INVALID), (dict(_3=0), INVALID), *nulls(0, 5, 6, 7), (dict(_1=60), INVALID)]
# ---- yolat_split_bf16x3_packed(W, ldw, N, K, row_scale, packed, stream)
PACK = (A, 64, 4, 64, None, A, None)
# ---- yolat_linear_x6(A, lda, M, K, Wp, shift, relu, N, out, ldo, stream)
LX = (A, 64, 4, 64, A, None, 0, 32, A, 32, None)
# ---- yolat_linear_x6_pre(Ap, M, K, Wp, shift, relu, N, out, ldo, stream)
LXP = (A, 4, 64, A, None, 0, 32, A, 32, None)
# ---- yolat_linear_fwd_rows_x6(A, lda, M, K, a_scale, a_shift, a_relu, W, ldw, bias, Nout, Y, ldy, stats, wsplit, stream)
LROWS = (A, 64, 10, 64, None, None, 0, A, 64, A, 64, A, 64, None, A, None)
# ---- yolat_node_uv_eval_x6(f_in, ld_f, s_in, ld_s, N, Wfr_h, Wfr_m, Wfr_l, tfr, Wn_h, Wn_m, Wn_l, tn_fold, UV, ld_uv, f_out,
#                            ld_fo, s_out, ld_so, stream)
NODE = (A, 64, A, 64, 10, A, A, A, A, A, A, A, A, A, 128, A, 64, A, 64, None)
# ---- yolat_fusion_pair_eval_x6_rn(A, lda, N, D, Wh, Wm, Wl, tcen, F, gamma_f, beta_f, node_seg, pool, ldpool, S, lds, P, Wsh,
#                                   Wsm, Wsl, tscen, gamma_s, beta_s, Ys, ldys, eps, stream)
RN = (A, 64, 10, 64, A, A, A, A, 64, None, None, A, A, 64, A, 64, 4, A, A, A, A, None, None, A, 64, 1e-5, None)

TABLE = [
    *rows("yolat_fusion_pair_eval_x6", PAIR, PAIR_SHARED + misaligned(4, 5, 6, 15, 16, 17)),
    *rows("yolat_fusion_pair_eval_f16x3", PAIR, PAIR_SHARED + misaligned(4, 5, 15, 16) + [
        (dict(_14=1 << 25, _20=128), UNSUPPORTED),       # P * ldys = 2^32 with P * ldpool = 2^31: the x6 call would launch
    ]),
    *rows("yolat_fusion_pair_eval_x6_act", PAIR_ACT, nulls(9, 11, 21)),
    *rows("yolat_fusion_pair_eval_f16x3_act", PAIR_ACT, nulls(9, 11, 21)),

    *rows("yolat_split_bf16x3", SPLIT, SPLIT_SHARED),
    *rows("yolat_split_f16x2", SPLIT, SPLIT_SHARED + [
        (dict(_2=E31), UNSUPPORTED), (dict(_3=E31, _1=E31), UNSUPPORTED),
    ]),
    *rows("yolat_split_bf16x3_packed", PACK, [
        (dict(_2=0), INVALID), (dict(_3=0), INVALID), *nulls(0, 5), (dict(_1=60), INVALID),
        (dict(_2=E31 - 32), INVALID), (dict(_3=E31, _1=E31), INVALID),
        (dict(_3=72, _1=72), UNSUPPORTED), *misaligned(5),
    ]),

    *rows("yolat_linear_x6", LX, [
        (dict(_2=0), INVALID), (dict(_7=0), INVALID), (dict(_3=0), INVALID), *nulls(0, 4, 8),
        (dict(_1=48), INVALID), (dict(_9=16), INVALID), (dict(_2=E31 - 32), INVALID), (dict(_7=E31 - 64, _9=E31), INVALID),
        (dict(_3=72, _1=72), UNSUPPORTED), (dict(_1=66), UNSUPPORTED), *misaligned(0, 4),
    ]),
    *rows("yolat_linear_x6_pre", LXP, [
        (dict(_1=0), INVALID), (dict(_6=0), INVALID), (dict(_2=0), INVALID), *nulls(0, 3, 7),
        (dict(_8=16), INVALID), (dict(_1=E31 - 32), INVALID), (dict(_6=E31 - 64, _8=E31), INVALID),
        (dict(_2=72), UNSUPPORTED), *misaligned(0, 3),
    ]),

    *rows("yolat_linear_fwd_rows_x6", LROWS, [
        (dict(_2=0), INVALID), *nulls(0, 7, 9, 11, 14), (dict(_1=60), INVALID), (dict(_8=60), INVALID),
        (dict(_12=60), INVALID),
        (dict(_4=A), INVALID), (dict(_5=A), INVALID), (dict(_6=1), INVALID),
        (dict(_3=96, _1=96, _8=96), UNSUPPORTED), (dict(_10=0), UNSUPPORTED), (dict(_10=32), UNSUPPORTED),
        (dict(_1=66), UNSUPPORTED), *misaligned(0, 14), (dict(_2=E31 - 256), UNSUPPORTED),
    ]),

    *rows("yolat_node_uv_eval_x6", NODE, [
        (dict(_4=0), INVALID), (dict(_4=E31 - 256), INVALID), *nulls(0, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 17),
        (dict(_1=60), INVALID), (dict(_3=60), INVALID), (dict(_14=124), INVALID), (dict(_16=60), INVALID),
        (dict(_18=60), INVALID),
        (dict(_1=66), UNSUPPORTED), (dict(_3=66), UNSUPPORTED), *misaligned(0, 2, 5, 6, 7, 9, 10, 11),
    ]),

    *rows("yolat_fusion_pair_eval_x6_rn", RN, [
        (dict(_2=0), INVALID), (dict(_16=0), INVALID), (dict(_8=0), INVALID),
        *nulls(0, 4, 5, 6, 7, 11, 12, 14, 17, 18, 19, 20, 23),
        (dict(_25=-1.0), INVALID), (dict(_25=float("nan")), INVALID),
        (dict(_9=A), INVALID), (dict(_10=A), INVALID), (dict(_21=A), INVALID), (dict(_22=A), INVALID),
        (dict(_1=60), INVALID), (dict(_15=60), INVALID), (dict(_13=60), INVALID), (dict(_24=60), INVALID),
        (dict(_3=96, _1=96, _15=96), UNSUPPORTED), (dict(_8=32), UNSUPPORTED),
        (dict(_1=66), UNSUPPORTED), (dict(_15=66), UNSUPPORTED), *misaligned(0, 14, 4, 5, 6, 17, 18, 19),
        (dict(_16=1 << 26), UNSUPPORTED),                # P * ldpool = 2^32
        (dict(_2=E31 - 256), UNSUPPORTED),               # N >= 2^31 - 2 * YOLAT_RN_ROWS
        (dict(_8=1 << 25, _13=1 << 25, _24=1 << 25), UNSUPPORTED),       # F * D = 2^31
    ]),
]


def test_the_table_covers_the_twelve_ops():
    assert len({fn for fn, _, _ in TABLE}) == 12


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_rejected_call_returns_its_code(row):
    fn, args, want = TABLE[row]
    assert getattr(_lib.lib, fn)(*args) == want, (fn, args)


# yolat_split_bf16x3_packed_elems(N, K) = cdiv(N, 32) * (K / 16) * 3 * 512, 0 for N <= 0 or K <= 0 (and so for K < 16)
PACKED_ELEMS = {
    (0, 64): 0, (-1, 64): 0, (4, 0): 0, (4, -16): 0, (4, 15): 0,
    (4, 16): 1536, (32, 16): 1536, (33, 16): 3072, (27, 31): 1536, (33, 64): 12288, (32, 2304): 221184,
    (512, 2304): 3538944,
}


@pytest.mark.parametrize("key", sorted(PACKED_ELEMS))
def test_packed_elems(key):
    assert _lib.lib.yolat_split_bf16x3_packed_elems(*key) == PACKED_ELEMS[key]
