// fx_rows.hpp — what the two-problem rows kernels k_fusion_rows_x6 (fusion_x6.hip) and k_fusion_rows_f16x3
// (fusion_f16x3.hip) have in common outside their bodies: the workgroup shape, the slopes argument, and the one launcher
// that picks an instantiation.  Of the bodies, the workgroup map and the W-tile movers (rownorm.hip's k_fusion_rows_rn
// uses the movers too) are TEXT the kernels include, fx_wg_map.inc and fx_w_movers.inc; the A prologue and the plain act
// store stay written out per kernel.  None of the four is a function here: each, as one, changed the instructions of
// every kernel that used it ("File layout of the rows kernels").
#pragma once
#include "internal.hpp"

// Threads per workgroup (32 rows per wave).  K = 128 (fusion blocks): 512 threads = 256 rows, one workgroup per CU (248
// registers, 105 KB of LDS).  K = 64 (node side, training Linear: one to three column tiles per workgroup, store-heavy):
// 256 threads = 128 rows and 75 KB of LDS, so that TWO workgroups share a CU and one's prologue / stores run under the
// other's MFMAs.
template <int KD> struct FxShape { static constexpr int T = KD == 64 ? 256 : 512, ROWS = T / 2; };
// ACT != 0: the activation-aware instantiation (leaky activations, act.hip) of the eval pair launch — act(y) = y > 0 ? y :
// a * y per element, signed pooling (segmax.hpp fx_segmax2_off_act) for the problem with seg, act in the plain store of
// the other.  The slopes (device pointers to one float each, read by every workgroup) are an argument only that
// instantiation has: FxSlopes<0> is empty, and nothing in the ACT == 0 code reads it.
template <int ACT> struct FxSlopes {};
template <> struct FxSlopes<1> { const float* s0; const float* s1; };

// The launcher.  Fam names a kernel family — FxX6 (fusion_x6.hip) or FxF16x3 (fusion_f16x3.hip): its problem type Prob and
// launch<KD, RIDER, ACT>(grid, stream, p0, p1, rider, slopes) — and the instantiation follows from D in {64, 128}, a rider
// with blocks, and the slopes (both or none).  These eight per family are all the instantiations there are; a
// single-problem user passes an empty rider and no slopes.
template <class Fam>
inline void fx_launch_rows(int64_t D, unsigned grid, const typename Fam::Prob& p0, const typename Fam::Prob& p1,
                           const PoolRider& rider, const float* slope_f, const float* slope_s, hipStream_t st) {
  const FxSlopes<0> none{};
  const FxSlopes<1> sl{slope_f, slope_s};
  switch ((D == 128 ? 4 : 0) | (rider.blocks > 0 ? 2 : 0) | (slope_f != nullptr ? 1 : 0)) {
    case 0: Fam::template launch<64, false, 0>(grid, st, p0, p1, rider, none); break;
    case 1: Fam::template launch<64, false, 1>(grid, st, p0, p1, rider, sl); break;
    case 2: Fam::template launch<64, true, 0>(grid, st, p0, p1, rider, none); break;
    case 3: Fam::template launch<64, true, 1>(grid, st, p0, p1, rider, sl); break;
    case 4: Fam::template launch<128, false, 0>(grid, st, p0, p1, rider, none); break;
    case 5: Fam::template launch<128, false, 1>(grid, st, p0, p1, rider, sl); break;
    case 6: Fam::template launch<128, true, 0>(grid, st, p0, p1, rider, none); break;
    case 7: Fam::template launch<128, true, 1>(grid, st, p0, p1, rider, sl); break;
  }
}
