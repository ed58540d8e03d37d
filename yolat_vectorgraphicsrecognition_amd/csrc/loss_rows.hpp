// loss_rows.hpp — the per-row device code of the classification loss, defined once for the two translation units
// that run it: loss_optim.hip (k_softmax_ce_rows / k_bce_rows + their final kernels: DetectionLoss, the training step)
// and evaluate.hip (k_eval_rows / k_eval_final: the loss of the rows an evaluation batch selects).  A row's loss term, the
// workgroup's fixed-order tree over 256 rows and the final fixed-order sum over the per-workgroup partials are the SAME
// text in both, so the two paths agree bit for bit wherever they see the same rows at the same tree positions.
#pragma once
#include "base.hpp"

// ------------------------------------------------------------------------------------------------
// The two row bodies are MACROS, not functions: a function is simplified on its own before it is inlined, and the rows
// kernels of loss_optim.hip then come out with other instructions than they had while the text stood in the kernel
// (commuted adds, another index computation for z[y]; profiles/evaluate_async_isa_identity.txt).  As text the compiler
// sees what it always saw, and there is still one definition.
//
// YL_CE_ROW_LOSS: nn.CrossEntropyLoss, one row held in registers (K <= KMAX: all loads independent, one expf per element).
// z: the row's logits; p: the row's index in labels and in dl, the gradient matrix (nullable, leading dimension lddl);
// P: the rows the mean is taken over (the gradient's 1 / P); row_loss: the float the term is assigned to.
// A label outside [0, K) (torch raises "Target out of bounds"; ignore_index is not used by the reference,
// architecture3cc_rpn_gp_iter2.py:363) must not become an out-of-bounds read: the loss is poisoned with NaN.
// ------------------------------------------------------------------------------------------------
#define YL_CE_ROW_LOSS(KMAX, z, K, labels, p, P, dl, lddl, row_loss)                      \
  {                                                                                       \
    float v[KMAX];                                                                        \
    _Pragma("unroll") for (int k = 0; k < KMAX; ++k) v[k] = z[k < K ? k : K - 1];         \
    float m = v[0];                                                                       \
    _Pragma("unroll") for (int k = 1; k < KMAX; ++k) m = fmaxf(m, v[k]);                  \
    float s = 0.f;                                                                        \
    _Pragma("unroll") for (int k = 0; k < KMAX; ++k) {                                    \
      v[k] = expf(v[k] - m);                                                              \
      s += (k < K) ? v[k] : 0.f;                                                          \
    }                                                                                     \
    const int64_t yl = labels[p];                                                         \
    const bool bad = yl < 0 || yl >= K;                                                   \
    const int y = bad ? 0 : (int)yl;                                                      \
    row_loss = bad ? __builtin_nanf("") : m + logf(s) - z[y];                             \
    if (dl != nullptr) {                                                                  \
      const float invs = 1.f / s, invP = 1.f / (float)P;                                  \
      float* d = dl + (long)p * lddl;                                                     \
      _Pragma("unroll") for (int k = 0; k < KMAX; ++k)                                    \
        if (k < K) d[k] = (v[k] * invs - (k == y ? 1.f : 0.f)) * invP;                    \
    }                                                                                     \
  }

// ------------------------------------------------------------------------------------------------
// classifier != 'softmax' (architecture3cc_rpn_gp_iter2.py:132-133,362-376): torch.sigmoid on the logits, nn.BCELoss
// (mean over all P*K elements) against the one-hot labels.  Every step is rounded to fp32 on its own, in torch's order:
//   p = 1 / (1 + exp(-z));  term = -max(log(p), -100) (target 1) or -max(log(1 - p), -100) (target 0)
//   q = p (1 - p);  dp = ((p - t) / max(q, 1e-12)) / n;  dz = dp q
// which is BCELoss' backward followed by sigmoid's — NOT the closed form (p - t) / n: where p rounds to exactly 1.0f or
// 0.0f the reference's gradient is 0 and a wrong element's loss term is 100, and that is kept.
// The fused entry point and the three separate ones run these same four functions, so they agree bit for bit.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float yl_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float yl_bce_term(float p, bool t) {
  return -(t ? fmaxf(logf(p), -100.f) : fmaxf(logf(1.f - p), -100.f));
}
__device__ __forceinline__ float yl_bce_dp(float p, bool t, float inv_n) {
  const float q = p * (1.f - p);
  return ((p - (t ? 1.f : 0.f)) / fmaxf(q, 1e-12f)) * inv_n;
}
__device__ __forceinline__ float yl_sigmoid_dz(float dp, float p) { return dp * (p * (1.f - p)); }

// One element of a row: in = logit (LOGITS) or probability; adds the loss term, writes prob (LOGITS only, nullable)
// and the gradient w.r.t. `in` (nullable).
template <bool LOGITS>
__device__ __forceinline__ float yl_bce_elem(float in, bool t, float inv_n, float* prob, float* dout) {
  const float p = LOGITS ? yl_sigmoid(in) : in;
  if (LOGITS && prob != nullptr) *prob = p;
  if (dout != nullptr) {
    const float dp = yl_bce_dp(p, t, inv_n);
    *dout = LOGITS ? yl_sigmoid_dz(dp, p) : dp;
  }
  return yl_bce_term(p, t);
}

// YL_BCE_ROW_LOSS: one row of the BCE loss.  KMAX > 0: K <= KMAX, the row is loaded into registers first (all loads
// independent); KMAX == 0: a plain loop over K.  The row's terms are added in ascending column order either way.  z: the
// row; p: its index in labels, in dout (the gradient, nullable) and in prob (the probabilities, LOGITS only, nullable).
// A label outside [0, K) matches no column (nothing is read through it); the loss is poisoned with NaN.
#define YL_BCE_ROW_LOSS(KMAX, LOGITS, z, K, labels, p, inv_n, dout, ldd, prob, ldp, row_loss)                             \
  {                                                                                                                       \
    const int64_t yl = labels[p];                                                                                         \
    const bool bad = yl < 0 || yl >= K;                                                                                   \
    const int y = bad ? -1 : (int)yl;                                                                                     \
    float* d = dout != nullptr ? dout + (long)p * ldd : nullptr;                                                          \
    float* pr = (LOGITS && prob != nullptr) ? prob + (long)p * ldp : nullptr;                                             \
    if (KMAX > 0) {                                                                                                       \
      float v[KMAX > 0 ? KMAX : 1];                                                                                       \
      _Pragma("unroll") for (int k = 0; k < KMAX; ++k) v[k] = z[k < K ? k : K - 1];                                       \
      _Pragma("unroll") for (int k = 0; k < KMAX; ++k)                                                                    \
        if (k < K) row_loss += yl_bce_elem<LOGITS>(v[k], k == y, inv_n, pr ? pr + k : nullptr, d ? d + k : nullptr);      \
    } else {                                                                                                              \
      for (int k = 0; k < K; ++k)                                                                                         \
        row_loss += yl_bce_elem<LOGITS>(z[k], k == y, inv_n, pr ? pr + k : nullptr, d ? d + k : nullptr);                 \
    }                                                                                                                     \
    if (bad) row_loss = __builtin_nanf("");                                                                               \
  }

// The 256 row terms of a workgroup, added in a fixed-order tree; thread 0 leaves the sum in out[0].  (The 1 KB of LDS is
// the function's own: every kernel that calls it gets the array, as if it had declared it.)
__device__ __forceinline__ void yl_rows_tree256(int tid, float row_loss, float* out) {
  __shared__ float red[256];
  red[tid] = row_loss;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

// The n per-workgroup sums, added in a fixed order by ONE 1024-thread workgroup: thread t adds work[t], work[t + 1024], ...
// then a tree; thread 0 hands the sum to fin(sum), which scales and stores it.
template <class Fin>
__device__ __forceinline__ void yl_partials_tree1024(const float* work, int n, int tid, Fin fin) {
  __shared__ float red[1024];
  float a = 0.f;
  for (int i = tid; i < n; i += 1024) a += work[i];
  red[tid] = a;
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) fin(red[0]);
}
