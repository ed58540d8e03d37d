"""CPU test (-m "not gpu") of the argument checks of the edge ops that have a bfloat16-storage twin (csrc/edge_ops.hip):
yolat_edge_uv_lin1_fwd[_h], yolat_csr_mean_fwd[_h], yolat_csr_mean_bwd[_h], yolat_edge_uv_sums[_h|_v].  Each pair shares
one host wrapper; the table below pins the return code of every rejected call — one row per term of every check, and
the rows where a twin answers differently from its fp32 form — so the shared wrapper cannot move a code.  The addresses
are fake: every row returns before a launch (a row that would launch has no place here), so no GPU is needed."""
import pytest

from yolat_vectorgraphicsrecognition_amd import _lib

INVALID, UNSUPPORTED, OK = -1, -2, 0
A = 0x10000          # 16-byte aligned
A8 = 0x10008         # 8-byte aligned only
A4 = 0x10004         # 4-byte aligned only
E31 = 1 << 31

TABLE = [
    # ---- yolat_edge_uv_lin1_fwd(UV, ld_uv, src, dst, attr, E, Wc4, b1, C, H1, ldh, stats, stream), fp32 and _h alike
    *[(fn, args, rc) for fn in ("yolat_edge_uv_lin1_fwd", "yolat_edge_uv_lin1_fwd_h") for args, rc in [
        ((A, 128, A, A, A, -1, A, A, 64, A, 64, A, None), INVALID),
        ((None, 128, A, A, A, 10, A, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, A, A, 10, None, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, A, A, 10, A, A, 32, A, 64, A, None), UNSUPPORTED),
        ((A, 128, None, None, None, 0, A, A, 32, None, 64, A, None), UNSUPPORTED),       # C is checked before E == 0
        ((A, 128, None, None, None, 0, A, None, 64, None, 0, None, None), OK),
        ((A, 128, None, A, A, 10, A, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, None, A, 10, A, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, A, None, 10, A, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, A, A, 10, A, A, 64, None, 64, A, None), INVALID),
        ((A, 128, A, A, A, E31, A, A, 64, A, 64, A, None), INVALID),
        ((A, 128, A, A, A, 10, A, A, 64, A, 60, A, None), INVALID),
        ((A, 127, A, A, A, 10, A, A, 64, A, 64, A, None), INVALID),
        ((A, 130, A, A, A, 10, A, A, 64, A, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A, 10, A, A, 64, A, 66, A, None), UNSUPPORTED),
        ((A8, 128, A, A, A, 10, A, A, 64, A, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A8, 10, A, A, 64, A, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A, 10, A8, A, 64, A, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A, 10, A, A, 64, A4, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A, 10, A, A8, 64, A, 64, A, None), UNSUPPORTED),
        ((A, 128, A, A, A, 10, A, A, 64, A, 64, A4, None), UNSUPPORTED),
    ]],
    # twins differ: fp32 rows of H1 are 16-byte aligned, bf16 rows 8-byte (the _h call would launch)
    ("yolat_edge_uv_lin1_fwd", (A, 128, A, A, A, 10, A, A, 64, A8, 64, A, None), UNSUPPORTED),

    # ---- yolat_csr_mean_fwd(H, ldh, C, h_scale, h_shift, h_relu, row_ptr, N, out, ldo, accumulate, stream)
    # fp32: whatever passes these checks launches (any C, any layout, H not looked at)
    ("yolat_csr_mean_fwd", (A, 64, 64, None, None, 0, A, 0, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 0, None, None, 0, A, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 64, None, None, 0, None, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 64, None, None, 0, A, 10, None, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 64, None, None, 0, A, 10, A, 60, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 64, A, None, 0, A, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd", (A, 64, 64, None, A, 0, A, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, A, 0, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (None, 64, 64, None, None, 0, A, 10, A, 64, 0, None), INVALID),       # twins differ: null H
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, None, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, A, 10, None, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, A, 10, A, 60, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (A, 60, 64, None, None, 0, A, 10, A, 64, 0, None), INVALID),          # twins differ: ldh < C
    ("yolat_csr_mean_fwd_h", (A, 64, 64, A, None, 0, A, 10, A, 64, 0, None), INVALID),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, A, 0, A, 10, A, 64, 0, None), INVALID),
    # twins differ: no scalar kernel behind the bf16 form (each of these launches in fp32, C = 0 apart: INVALID above)
    ("yolat_csr_mean_fwd_h", (A, 64, 32, None, None, 0, A, 10, A, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 64, 0, None, None, 0, A, 10, A, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 66, 64, None, None, 0, A, 10, A, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, A, 10, A, 66, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A4, 64, 64, None, None, 0, A, 10, A, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, None, None, 0, A, 10, A8, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, A8, A, 0, A, 10, A, 64, 0, None), UNSUPPORTED),
    ("yolat_csr_mean_fwd_h", (A, 64, 64, A, A8, 0, A, 10, A, 64, 0, None), UNSUPPORTED),

    # ---- yolat_csr_mean_bwd(dOut, lddo, C, row_ptr, dst, E, dM, lddm, stream)
    *[(fn, args, rc) for fn in ("yolat_csr_mean_bwd", "yolat_csr_mean_bwd_h") for args, rc in [
        ((A, 64, 64, A, A, -1, A, 64, None), INVALID),
        ((None, 64, 64, A, A, 10, A, 64, None), INVALID),
        ((A, 64, 64, None, A, 10, A, 64, None), INVALID),
        ((A, 64, 64, A, None, 0, None, 0, None), OK),
        ((A, 64, 64, A, None, 10, A, 64, None), INVALID),
        ((A, 64, 64, A, A, 10, None, 64, None), INVALID),
        ((A, 64, 64, A, A, 10, A, 60, None), INVALID),
    ]],
    # twins differ: C <= 0 is invalid in fp32; the bf16 form does not look at C before E == 0 and the layout check
    ("yolat_csr_mean_bwd", (A, 64, 0, A, A, 10, A, 64, None), INVALID),
    ("yolat_csr_mean_bwd", (A, 64, 0, A, None, 0, None, 0, None), INVALID),
    ("yolat_csr_mean_bwd_h", (A, 64, 0, A, A, 10, A, 64, None), UNSUPPORTED),
    ("yolat_csr_mean_bwd_h", (A, 64, 0, A, None, 0, None, 0, None), OK),
    # twins differ: no scalar kernel behind the bf16 form (each of these launches in fp32)
    ("yolat_csr_mean_bwd_h", (A, 64, 32, A, A, 10, A, 64, None), UNSUPPORTED),
    ("yolat_csr_mean_bwd_h", (A, 66, 64, A, A, 10, A, 64, None), UNSUPPORTED),
    ("yolat_csr_mean_bwd_h", (A, 64, 64, A, A, 10, A, 66, None), UNSUPPORTED),
    ("yolat_csr_mean_bwd_h", (A8, 64, 64, A, A, 10, A, 64, None), UNSUPPORTED),
    ("yolat_csr_mean_bwd_h", (A, 64, 64, A, A, 10, A4, 64, None), UNSUPPORTED),

    # ---- yolat_edge_uv_sums(dH1, ldh, row_ptr, col_ptr, slots, N, C, dUV, ld_uv, stream), fp32 and _h alike
    *[(fn, args, rc) for fn in ("yolat_edge_uv_sums", "yolat_edge_uv_sums_h") for args, rc in [
        ((A, 64, A, A, A, 0, 64, A, 128, None), INVALID),
        ((None, 64, A, A, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, None, A, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, None, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, A, None, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, A, A, 10, 64, None, 128, None), INVALID),
        ((A, 60, A, A, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, A, A, 10, 64, A, 127, None), INVALID),
        ((A, 64, A, A, A, 10, 32, A, 128, None), UNSUPPORTED),
        ((A, 66, A, A, A, 10, 64, A, 128, None), UNSUPPORTED),
        ((A, 64, A, A, A, 10, 64, A, 130, None), UNSUPPORTED),
        ((A4, 64, A, A, A, 10, 64, A, 128, None), UNSUPPORTED),
        ((A, 64, A, A, A, 10, 64, A8, 128, None), UNSUPPORTED),
    ]],
    ("yolat_edge_uv_sums", (A8, 64, A, A, A, 10, 64, A, 128, None), UNSUPPORTED),      # twins differ: 16- / 8-byte rows
    # ---- yolat_edge_uv_sums_v(dH1, ldh, half, col_ptr, slots, N, C, dUV, ld_uv, stream): no row_ptr to check
    *[("yolat_edge_uv_sums_v", args[:2] + (half,) + args[2:], rc) for half in (0, 1) for args, rc in [
        ((A, 64, A, A, 0, 64, A, 128, None), INVALID),
        ((None, 64, A, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, None, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, None, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, A, 10, 64, None, 128, None), INVALID),
        ((A, 60, A, A, 10, 64, A, 128, None), INVALID),
        ((A, 64, A, A, 10, 64, A, 127, None), INVALID),
        ((A, 64, A, A, 10, 32, A, 128, None), UNSUPPORTED),
        ((A, 66, A, A, 10, 64, A, 128, None), UNSUPPORTED),
        ((A, 64, A, A, 10, 64, A, 130, None), UNSUPPORTED),
        ((A4, 64, A, A, 10, 64, A, 128, None), UNSUPPORTED),
        ((A, 64, A, A, 10, 64, A8, 128, None), UNSUPPORTED),
    ]],
    ("yolat_edge_uv_sums_v", (A8, 64, 0, A, A, 10, 64, A, 128, None), UNSUPPORTED),    # half = 0: 16-byte rows
]


def test_the_table_covers_the_nine_wrappers():
    assert len({fn for fn, _, _ in TABLE}) == 9


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_rejected_call_returns_its_code(row):
    fn, args, want = TABLE[row]
    assert getattr(_lib.lib, fn)(*args) == want, (fn, args)
