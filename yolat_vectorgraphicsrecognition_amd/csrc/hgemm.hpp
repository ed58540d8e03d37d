// hgemm.hpp — the tile GEMM of the bf16-storage paths: operand types, LDS tile, kernels, launcher.  Every k_hgemm / k_hgemm_act
// instance lives in ONE translation unit, bf16_eval.hip (a second one gives an instance a different address arithmetic,
// DESIGN.md §3): a file that only builds operands for a launch made there defines YL_HGEMM_TYPES_ONLY and sees no kernel.
#pragma once
#include "operands.hpp"
#include "epilogue.hpp"
#include <type_traits>

typedef unsigned short u16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------
// NT GEMM on bf16 MFMAs:  Y[M,N] = epi( A[M,K] . B[N,K]^T ),  K % 64 == 0.
// 256 threads = 2x2 waves, wave tile (32 TM) x (32 TN); K step 64 bf16 = 128 B per row.  LDS rows are padded
// to 144 B so that both the 16-byte staging writes (8 lanes = one row) and the 16-byte fragment reads
// (8 consecutive rows at one k offset) hit 8 distinct 16-byte bank groups.
//   MFMA operand layout: A/B lane l holds the 8 consecutive k = 16 ks + 8 (l>>5) .. +7 of row / column l&31;
//   C/D layout as for the fp32 MFMA, so wave_epilogue (epilogue.hpp) is shared with the fp32 kernels.
// A operand: bf16 rows (HOp) or fp32 rows converted while staging (FOp); B operand: bf16 weight rows.
// Rows beyond M / N are clamped (their outputs are masked by the epilogue).
// ------------------------------------------------------------------------------------------------
struct HOp {
  const u16* p; long ld; int rows;
  static constexpr int NR = 1;
  __device__ __forceinline__ void load(int r, int k, u32x4* raw) const {
    raw[0] = *reinterpret_cast<const u32x4*>(p + (long)yl_min(r, rows - 1) * ld + k);
  }
  static __device__ __forceinline__ u32x4 pack(const u32x4* raw) { return raw[0]; }
};
struct FOp {
  const float* p; long ld; int rows;
  static constexpr int NR = 2;
  __device__ __forceinline__ void load(int r, int k, u32x4* raw) const {
    const float* q = p + (long)yl_min(r, rows - 1) * ld + k;
    raw[0] = *reinterpret_cast<const u32x4*>(q);
    raw[1] = *reinterpret_cast<const u32x4*>(q + 4);
  }
  static __device__ __forceinline__ u32x4 pack(const u32x4* raw) {
    u32x4 o;
    o.x = yl_pack_bf16(__uint_as_float(raw[0].x), __uint_as_float(raw[0].y));
    o.y = yl_pack_bf16(__uint_as_float(raw[0].z), __uint_as_float(raw[0].w));
    o.z = yl_pack_bf16(__uint_as_float(raw[1].x), __uint_as_float(raw[1].y));
    o.w = yl_pack_bf16(__uint_as_float(raw[1].z), __uint_as_float(raw[1].w));
    return o;
  }
};

// bf16 rows with the producer's BatchNorm + ReLU applied while staging (training with bf16 storage: the consumer of
// a lazily normalised activation): widen, fma with the per-column (scale, shift), floor, round back to bf16.
struct HProOp {
  const u16* p; long ld; int rows;
  const float* scale; const float* shift; float floor;
  static constexpr int NR = 1;
  __device__ __forceinline__ void load(int r, int k, u32x4* raw) const {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p + (long)yl_min(r, rows - 1) * ld + k);
    const float4 s0 = *reinterpret_cast<const float4*>(scale + k), s1 = *reinterpret_cast<const float4*>(scale + k + 4);
    const float4 h0 = *reinterpret_cast<const float4*>(shift + k), h1 = *reinterpret_cast<const float4*>(shift + k + 4);
    u32x4 o;
    o.x = yl_pack_bf16(fmaxf(fmaf(yl_bf16_lo(v.x), s0.x, h0.x), floor), fmaxf(fmaf(yl_bf16_hi(v.x), s0.y, h0.y), floor));
    o.y = yl_pack_bf16(fmaxf(fmaf(yl_bf16_lo(v.y), s0.z, h0.z), floor), fmaxf(fmaf(yl_bf16_hi(v.y), s0.w, h0.w), floor));
    o.z = yl_pack_bf16(fmaxf(fmaf(yl_bf16_lo(v.z), s1.x, h1.x), floor), fmaxf(fmaf(yl_bf16_hi(v.z), s1.y, h1.y), floor));
    o.w = yl_pack_bf16(fmaxf(fmaf(yl_bf16_lo(v.w), s1.z, h1.z), floor), fmaxf(fmaf(yl_bf16_hi(v.w), s1.w, h1.w), floor));
    raw[0] = o;
  }
  static __device__ __forceinline__ u32x4 pack(const u32x4* raw) { return raw[0]; }
};

constexpr int YL_HRS = 72;   // LDS row stride in bf16 elements (144 B)
template <int TM, int TN> struct HTileSmem { static constexpr int elems = 64 * (TM + TN) * YL_HRS; };

static Epilogue plain_epilogue() {
  Epilogue e;
  e.bias = nullptr; e.scale = nullptr; e.shift = nullptr; e.relu = 0;
  e.Y = nullptr; e.ldy = 0; e.accumulate = 0; e.stats = nullptr; e.seg = nullptr; e.pool = nullptr; e.ldpool = 0;
  return e;
}

#ifndef YL_HGEMM_TYPES_ONLY
// wave_epilogue (epilogue.hpp) for a leaky activation (act.hip): v = act((acc + bias) * scale + shift) with
// act(y) = y > 0 ? y : a * y computed in fp32 BEFORE the store, so a bf16 output is rounded once, like the ReLU one.  The
// plain-store forms only (ep.Yh bf16 or ep.Y fp32, through the wave's staging region where the tile is whole and aligned,
// element by element otherwise); a NaN stays a NaN.
__device__ __forceinline__ void wave_epilogue_act(f32x16 acc, int row_base, int col, int lhi, const Epilogue& ep, int M, int N,
                                                  const EpiPre& pre, float* stage, float a) {
  const bool col_ok = col < N;
  const float bv = ep.bias != nullptr ? pre.bias : 0.f, sc = pre.sc, sh = pre.sh;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float y = fmaf(acc[r] + bv, sc, sh);
    acc[r] = y > 0.f ? y : a * y;
  }
  const int l31s = threadIdx.x & 31, lane = threadIdx.x & 63, col_base = col - l31s;
  if (yl_stage_ok(ep, row_base, col_base, M, N)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * lhi) * YL_STAGE_LD + l31s] = acc[r];
    if (ep.Yh != nullptr) yl_stage_store_bf16(stage, ep, row_base, col_base, lane);
    else yl_stage_store_f32(stage, ep, row_base, col_base, lane);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    if (col_ok && row < M) {
      if (ep.Yh != nullptr) ep.Yh[(long)row * ep.ldy + col] = (u16)(yl_pack_bf16(acc[r], 0.f) & 0xFFFFu);
      else ep.Y[(long)row * ep.ldy + col] = acc[r];
    }
  }
}

// ACT = 1: the epilogue is wave_epilogue_act with the slope read from *slope; nothing else differs
template <int TM, int TN, class AL, int ACT = 0>
__device__ __forceinline__ void hgemm_tile(const AL& A, const HOp& B, const Epilogue& ep, int M, int N, int K, int rt_,
                                           int ct_, u16* smem, const float* slope = nullptr) {
  constexpr int BM = 64 * TM, BN = 64 * TN, NA = 2 * TM, NB = 2 * TN;   // 16-byte slots per thread per K step
  u16* As = smem;
  u16* Bs = smem + BM * YL_HRS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt_ * BM, col0 = ct_ * BN;
  const int sr = tid >> 3, sc = (tid & 7) * 8;          // staging role: row sr (+32 per slot), k chunk sc

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // PF K steps of operands in flight (round 5): with one, a long-K classifier tile kept 64 KB per CU on the way and ran at
  // the latency of its loads (1.2 us per K step for 256 cycles of MFMA per wave)
  constexpr int PF = 2;        // (3: 150 registers, no faster)
  u32x4 ra[PF][NA * AL::NR], rb[PF][NB];
#pragma unroll
  for (int q = 0; q < PF; ++q)
    if (64 * q < K) {
#pragma unroll
      for (int t = 0; t < NA; ++t) A.load(row0 + sr + 32 * t, 64 * q + sc, ra[q] + t * AL::NR);
#pragma unroll
      for (int t = 0; t < NB; ++t) B.load(col0 + sr + 32 * t, 64 * q + sc, rb[q] + t);
    }

  EpiPre pre[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      pre[i][j] = epi_prefetch(ep, row0 + (wm * TM + i) * 32, col0 + (wn * TN + j) * 32 + l31, M, N);
  float act_a = 0.f;
  if constexpr (ACT != 0) act_a = *slope;               // with the epilogue constants: its latency hides under the K loop

  // one K step: stage the registers of step k0, refill them with step k0 + 64 PF, MFMAs
  auto kstep = [&](int k0, u32x4* qa, u32x4* qb) {
#pragma unroll
    for (int t = 0; t < NA; ++t)
      *reinterpret_cast<u32x4*>(As + (sr + 32 * t) * YL_HRS + sc) = AL::pack(qa + t * AL::NR);
#pragma unroll
    for (int t = 0; t < NB; ++t) *reinterpret_cast<u32x4*>(Bs + (sr + 32 * t) * YL_HRS + sc) = qb[t];
    __syncthreads();
    if (k0 + 64 * PF < K) {                 // PF steps ahead, in flight while the MFMAs below run
#pragma unroll
      for (int t = 0; t < NA; ++t) A.load(row0 + sr + 32 * t, k0 + 64 * PF + sc, qa + t * AL::NR);
#pragma unroll
      for (int t = 0; t < NB; ++t) B.load(col0 + sr + 32 * t, k0 + 64 * PF + sc, qb + t);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(As + ((wm * TM + i) * 32 + l31) * YL_HRS + ks * 16 + lhi * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(Bs + ((wn * TN + j) * 32 + l31) * YL_HRS + ks * 16 + lhi * 8);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  };
  for (int k0 = 0; k0 < K; k0 += 64 * PF) {
#pragma unroll
    for (int q = 0; q < PF; ++q)
      if (k0 + 64 * q < K) kstep(k0 + 64 * q, ra[q], rb[q]);
  }
  static_assert(TM <= 2 && TN <= 2, "epilogue expansion covers up to 2x2 sub-tiles");
  // the operand tiles are dead after the loop's closing barrier: every wave stages its stores in its own 4.5 KB of them
  static_assert(HTileSmem<TM, TN>::elems * 2 >= 4 * 32 * YL_STAGE_LD * 4, "LDS too small for the store staging");
  float* stage = reinterpret_cast<float*>(smem) + wave * (32 * YL_STAGE_LD);
#define YL_EPI(i, j)                                                                                                 \
  if constexpr ((i) < TM && (j) < TN) {                                                                              \
    const int rb_ = row0 + (wm * TM + (i)) * 32, c_ = col0 + (wn * TN + (j)) * 32 + l31;                             \
    if constexpr (ACT != 0) wave_epilogue_act(acc[i][j], rb_, c_, lhi, ep, M, N, pre[i][j], stage, act_a);           \
    else wave_epilogue(acc[i][j], rb_, c_, lhi, ep, M, N, pre[i][j], stage);                                         \
  }
  YL_EPI(0, 0) YL_EPI(0, 1) YL_EPI(1, 0) YL_EPI(1, 1)
#undef YL_EPI
}

template <int TM, int TN, class AL>
static __global__ void __launch_bounds__(256) k_hgemm(AL A, HOp B, Epilogue ep, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) u16 smem[HTileSmem<TM, TN>::elems];
  int rt_, ct_;
  yl_xcd_tile(rt_, ct_);
  hgemm_tile<TM, TN, AL>(A, B, ep, M, N, K, rt_, ct_, smem);
}
// the same tiles with the leaky activation in the epilogue (prediction_cls.0 / .1, fusion_block_super of a leaky model)
template <int TM, int TN, class AL>
static __global__ void __launch_bounds__(256) k_hgemm_act(AL A, HOp B, Epilogue ep, int M, int N, int K, const float* slope) {
  __shared__ __attribute__((aligned(16))) u16 smem[HTileSmem<TM, TN>::elems];
  int rt_, ct_;
  yl_xcd_tile(rt_, ct_);
  hgemm_tile<TM, TN, AL, 1>(A, B, ep, M, N, K, rt_, ct_, smem, slope);
}

// slope != nullptr: the leaky activation in the epilogue (k_hgemm_act), read from *slope by the launch.  *tile_form
// (optional) names the tile: 0 = 64 x 64, 1 = 64 x 128
template <class AL>
static int launch_hgemm(const AL& A, const HOp& B, const Epilogue& ep, long M, long N, long K, hipStream_t st,
                 int* tile_form = nullptr, const float* slope = nullptr) {
  if (K % 64 != 0 || M <= 0 || N <= 0) return YOLAT_E_UNSUPPORTED;
  // 64x128 tiles once they still fill the GPU (cfg 5 classifier 1: 55 -> 45 us)
  const bool wide = N % 128 == 0 && (long)yl_cdiv(M, 64) * (N / 128) >= 256;
  if (tile_form != nullptr) *tile_form = wide ? 1 : 0;
  const dim3 grid(yl_cdiv(M, 64), wide ? N / 128 : yl_cdiv(N, 64));
  auto go = [&](auto kern, auto... more) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, A, B, ep, (int)M, (int)N, (int)K, more...);
  };
  if (slope == nullptr) {
    if (wide) go(k_hgemm<1, 2, AL>);
    else go(k_hgemm<1, 1, AL>);
  } else if constexpr (std::is_same<AL, HProOp>::value) {
    return YOLAT_E_UNSUPPORTED;       // (no leaky consumer behind the BatchNorm prologue: no such instance)
  } else {
    if (wide) go(k_hgemm_act<1, 2, AL>, slope);
    else go(k_hgemm_act<1, 1, AL>, slope);
  }
  YL_LAUNCH_CHECK();
  return 0;
}
#endif  // YL_HGEMM_TYPES_ONLY
