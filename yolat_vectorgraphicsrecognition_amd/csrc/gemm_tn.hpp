// gemm_tn.hpp — the TN GEMM of the weight gradients and the fixed-order reduction of its split partials.
#pragma once
#include "operands.hpp"

// ------------------------------------------------------------------------------------------------
// TN GEMM (weight gradients):  P[s][n][k] = sum_{r in split s} Y[r][n] * A[r][k]
// Output tile 64(n) x 64(k); 64 rows per LDS stage (32 MFMAs per wave between barriers; 32-row stages left the
// N-row weight gradients latency bound: 97 us for [64,64] over 200 k rows); grid = (n tiles, k tiles, splits).
// ------------------------------------------------------------------------------------------------
template <class YL, class AL>
__global__ void __launch_bounds__(256) k_gemm_tn(YL Yop, AL Aop, float* partial, float* dbpart,
                                                  int M, int Nout, int K, int rows_per_split) {
  constexpr int BR = 64, BT = 64, NT = BR * 16 / 256;   // rows per LDS stage, tile edge, float4 slots per thread
  __shared__ __attribute__((aligned(16))) float Ys[BR][BT];
  __shared__ __attribute__((aligned(16))) float As[BR][BT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int n0 = blockIdx.x * BT, k0 = blockIdx.y * BT, s = blockIdx.z;
  const int r_begin = s * rows_per_split;
  int r_end = r_begin + rows_per_split;
  if (r_end > M) r_end = M;
  const bool fastY = (Yop.vec != 0) && (n0 + BT <= Nout);
  const bool fastA = (Aop.vec != 0) && (k0 + BT <= K);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float dbacc = 0.f;
  const bool do_db = (dbpart != nullptr) && (blockIdx.y == 0);

  float ry[NT][4], rx[NT][4];
  auto fetch = [&](int r0) {
    if (fastY) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int i = tid + t * 256;
        Yop.template load4<true>(r0 + i / 16, n0 + 4 * (i % 16), ry[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int i = tid + t * 256;
        Yop.template load4<false>(r0 + i / 16, n0 + 4 * (i % 16), ry[t]);
      }
    }
    if (fastA) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int i = tid + t * 256;
        Aop.template load4<true>(r0 + i / 16, k0 + 4 * (i % 16), rx[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int i = tid + t * 256;
        Aop.template load4<false>(r0 + i / 16, k0 + 4 * (i % 16), rx[t]);
      }
    }
  };

  if (r_begin < r_end) fetch(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += BR) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = tid + t * 256;
      const int r = i / 16, q = i % 16;
      const bool ok = (r0 + r) < r_end;          // rows are the reduction dimension: mask them
      *reinterpret_cast<float4*>(&Ys[r][4 * q]) =
          make_float4(ok ? ry[t][0] : 0.f, ok ? ry[t][1] : 0.f, ok ? ry[t][2] : 0.f, ok ? ry[t][3] : 0.f);
      *reinterpret_cast<float4*>(&As[r][4 * q]) =
          make_float4(ok ? rx[t][0] : 0.f, ok ? rx[t][1] : 0.f, ok ? rx[t][2] : 0.f, ok ? rx[t][3] : 0.f);
    }
    __syncthreads();
    if (r0 + BR < r_end) fetch(r0 + BR);
#pragma unroll
    for (int rr = 0; rr < BR; rr += 2) {
      const float a = Ys[rr + lhi][wm * 32 + l31];
      const float b = As[rr + lhi][wn * 32 + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (do_db && tid < BT) {
#pragma unroll
      for (int rr = 0; rr < BR; ++rr) dbacc += Ys[rr][tid];
    }
    __syncthreads();
  }
  float* P = partial + (long)s * Nout * K;
  const int kc = k0 + wn * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    if (n < Nout && kc < K) P[(long)n * K + kc] = acc[r];
  }
  if (do_db && tid < BT && n0 + tid < Nout) dbpart[(long)s * Nout + n0 + tid] = dbacc;
}

// dst[i] (+)= sum_s partial[s][i]   (fixed order: 8 contiguous split groups summed in order, then the 8
// group sums in order).  32 consecutive elements x 8 split groups per workgroup; 8 independent loads in
// flight per thread — a one-thread-per-element loop over S=512 splits is a chain of 512 dependent
// L2 round trips (130 us for a 64x64 weight).
__device__ __forceinline__ void reduce_splits_body(long blk, const float* partial, long elems, int S, float* dst,
                                                   long ld_dst, int cols, int accumulate) {
  __shared__ float gs[8][33];
  const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long i = blk * 32 + e;
  const int per = (S + 7) / 8;
  const int t0 = g * per, t1 = (t0 + per < S) ? t0 + per : S;
  float s = 0.f;
  if (i < elems) {
    const float* p = partial + i;
    int t = t0;
    for (; t + 8 <= t1; t += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(long)(t + j) * elems];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; t < t1; ++t) s += p[(long)t * elems];
  }
  gs[g][e] = s;
  __syncthreads();
  if (g == 0 && i < elems) {
    float tot = gs[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) tot += gs[k][e];
    float* d = dst + (i / cols) * ld_dst + (i % cols);
    if (accumulate) tot += *d;
    *d = tot;
  }
}
static __global__ void __launch_bounds__(256) k_reduce_splits(const float* partial, long elems, int S,
                                                              float* dst, long ld_dst, int cols,
                                                              int accumulate) {
  reduce_splits_body(blockIdx.x, partial, elems, S, dst, ld_dst, cols, accumulate);
}
// two reductions with the same split count in one launch (a weight gradient and its bias gradient: the second one is a
// handful of workgroups that used to be a ~5 us launch of their own)
static __global__ void __launch_bounds__(256) k_reduce_splits2(const float* pa, long ea, float* da, long lda, int ca,
                                                               const float* pb, long eb, float* db, long ldb, int cb,
                                                               int S, int accumulate, int blocks_a) {
  if ((int)blockIdx.x < blocks_a) reduce_splits_body(blockIdx.x, pa, ea, S, da, lda, ca, accumulate);
  else reduce_splits_body(blockIdx.x - blocks_a, pb, eb, S, db, ldb, cb, accumulate);
}
// dW (+)= sum of `partial` [S][Nout*K];  db (+)= sum of `dbpart` [S][Nout] when db != NULL
static inline void yl_reduce_dw_db(hipStream_t st, const float* partial, long elems, int S, float* dW, long lddw, int K,
                                   const float* dbpart, float* db, long Nout, int accumulate) {
  const int ba = yl_cdiv(elems, 32);
  if (db != nullptr) {
    hipLaunchKernelGGL(k_reduce_splits2, dim3(ba + yl_cdiv(Nout, 32)), dim3(256), 0, st, partial, elems, dW, lddw, K,
                       dbpart, Nout, db, Nout, (int)Nout, S, accumulate, ba);
  } else {
    hipLaunchKernelGGL(k_reduce_splits, dim3(ba), dim3(256), 0, st, partial, elems, S, dW, lddw, K, accumulate);
  }
}

struct TnPlan { int S; int rows_per_split; };
static inline TnPlan yl_tn_plan(long M, long Nout, long K) {
  const long tiles = (long)yl_cdiv(Nout, 64) * yl_cdiv(K, 64);
  long S = 1024 / tiles;
  if (S < 1) S = 1;
  if (S > 512) S = 512;
  long rps = (M + S - 1) / S;
  rps = ((rps + 31) / 32) * 32;
  if (rps < 64) rps = 64;
  S = (M + rps - 1) / rps;
  if (S < 1) S = 1;
  TnPlan p; p.S = (int)S; p.rows_per_split = (int)rps;
  return p;
}
