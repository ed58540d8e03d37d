// fx_wg_map.inc — workgroup -> (problem, logical index) of the two-problem rows launch, included as TEXT at the top of
// k_fusion_rows_x6 (fusion_x6.hip) and k_fusion_rows_f16x3 (fusion_f16x3.hip): the one copy of the mapping.  In scope:
// p0, p1 (tm, groups, full), rider, RIDER, T, tid.  It defines n1, n1p, id, n0t, n0, logical, whole and small, and
// returns from the kernel in a rider workgroup and in a padding workgroup; the kernel then picks the problem's fields
// by `small` and turns (logical, whole) into its row tile and column tiles.
// Text, not a function (gemm_sk_tile.inc's reason): behind a __device__ function that returns (small, rt, ct0, ngl) every
// instance of both kernels came out with other instructions — tools/kernel_isa_diff.py must say SAME for them.
  // the small problem's workgroups come first (padded to a multiple of 8 so that the big problem keeps its
  // id % 8 = XCD alignment): they start with the first round of workgroups instead of forming a tail
  const int n1 = p1.tm * p1.groups, n1p = (n1 + 7) & ~7;
  const int id = blockIdx.x;
  // workgroups past both problems: pooling-prologue rider (internal.hpp; reads A like the GEMM, writes columns of the
  // pooled rows that nothing in this launch reads)
  // the big problem: p0.full whole-row-tile workgroups first, then the remaining row tiles split into column groups
  const int n0t = (p0.tm - p0.full) * p0.groups, n0 = p0.full + n0t;
  if constexpr (RIDER) {
    if (id >= n1p + n0) {
      yl_pool_rider(rider, id - (n1p + n0), rider.blocks, tid, T);
      return;
    }
  }
  int logical;
  bool whole = false;
  if (id < n1p) {
    if (id >= n1) return;
    logical = id;
  } else if (id - n1p < p0.full) {
    logical = id - n1p;
    whole = true;
  } else {
    // (row tile, column group) pairs, column group fastest, dealt to the XCDs in contiguous ranges
    const int j0 = id - n1p - p0.full;
    const int chunk = n0t >> 3, rem = n0t & 7;
    const int xcd = j0 & 7, slot = j0 >> 3;
    logical = xcd * chunk + (xcd < rem ? xcd : rem) + slot;
  }
  const bool small = id < n1p;
