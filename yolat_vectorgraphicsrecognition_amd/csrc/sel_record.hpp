// sel_record.hpp — yolat_predict_select's record as the kernels address it (layout: include/yolat_hip.h, ABI 6 comment)
#pragma once
#include "base.hpp"
constexpr int YL_SEL_TOTAL = 0, YL_SEL_TREE = 1, YL_SEL_STATUS = 2, YL_SEL_HEAD = 4;      // head words; [3] is spare
template <class I> __host__ __device__ __forceinline__ I* yl_sel_image_off(I* sel) { return sel + YL_SEL_HEAD; }   // [B + 1]
template <class I> __host__ __device__ __forceinline__ I* yl_sel_rows(I* sel, int B) { return sel + YL_SEL_HEAD + B + 1; }
// sel, image_ptr and gt_ptr entries are read through this: whatever the array holds, every index derived from it is in range
__device__ __forceinline__ int yl_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// THE arg-max of a logits row, for the selection's has_object (k_predict_select) and the evaluation's top-1 (k_eval_rows):
// torch's max(1)[1], which the two-pass path and the reference take — the first index of the row maximum, a NaN counting
// as the maximum (so the first NaN of a row that holds one)
__device__ __forceinline__ int yl_argmax_row(const float* z, int K) {
  float best = z[0];
  int arg = 0;
  for (int c = 1; c < K; ++c) {
    const float x = z[c];
    if (best == best && (x > best || x != x)) { best = x; arg = c; }
  }
  return arg;
}
// a tree of at least min_B images that brings every array its sizes call for
static inline bool yl_predict_tree_ok(const yolat_predict_tree& t, int64_t min_B) {
  return t.R >= 0 && t.Ctot >= 0 && t.B >= min_B && t.image_root_ptr && t.child_ptr &&
         (t.R == 0 || (t.root_row && t.root_range)) && (t.Ctot == 0 || (t.child_row && t.child_range));
}
