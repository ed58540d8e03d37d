// epilogue.hpp — the epilogue of one 32x32 MFMA sub-tile: bias / BatchNorm statistics / scale-shift-ReLU / store,
// with the fused pooling, CSR-mean and bf16-storage variants.
#pragma once
#include "operands.hpp"

// ------------------------------------------------------------------------------------------------
// Epilogue of the NT GEMM
// ------------------------------------------------------------------------------------------------
struct Epilogue {
  const float* bias;   // nullable [N]
  const float* scale;  // nullable [N]
  const float* shift;
  int relu;
  float* Y;
  long ldy;
  int accumulate;
  float* stats;  // nullable: float2 [ceil(M/32)][N]  (sum, M2) of (acc + bias) per 32-row group
  // fused per-proposal max pooling (eval): when seg != nullptr the tile is NOT stored; instead
  // pool[seg[row]][col] = max(pool, value) with integer atomicMax on the float bits (values are
  // post-ReLU, i.e. >= 0, so int order == float order and max is exact and order-independent).
  const int* seg;  // nullable [M]
  float* pool;
  long ldpool;
  // training-mode fused pooling (fusion_train.hip): when key64 != nullptr the tile is not stored; for every
  // (segment, column) the row with the largest s*z (s = sign of `scale`, z = acc + bias) is recorded as
  //   key = orderable(s*z) << 32 | ~row     via 64-bit atomicMax  (ties -> lowest row)
  unsigned long long* key64 = nullptr;
  // fused CSR mean aggregation (eval node-side kernel): when agg != nullptr the value stored for row n is
  //   epi(acc)[n] + mean_{q in [agg_ptr[n], agg_ptr[n+1])} agg[q, col]      (ascending q, like k_csr_mean_fwd)
  const float* agg = nullptr;
  long ldagg = 0;
  const int* agg_ptr = nullptr;
  int agg_rows = 0;     // number of rows of agg (E), for address clamping
  // bf16 storage mode (bf16_eval.hip): when Yh != nullptr the tile is stored as bfloat16 (round-to-nearest-even)
  // at Yh[row*ldy + col] instead of fp32 at Y; ldy even, Yh 4-byte aligned.  Not combined with accumulate / agg.
  unsigned short* Yh = nullptr;
};

// Epilogue of one 32x32 MFMA sub-tile held by one wave (C/D layout: col = lane&31,
// row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)).  Everything is wave-local: the training-mode BatchNorm
// partial statistics of the 32-row group (sum, M2 around the group mean) need one cross-half
// shuffle and no LDS, and are written once per (32-row group, column) => deterministic.
// Per-column epilogue constants and the tile's segment ids, loaded at kernel START so their latency hides
// under the K loop (a dependent load after the last MFMA costs ~1-2k cycles of a 4k-cycle K=128 tile).
struct EpiPre { float bias, sc, sh; int segv; };
__device__ __forceinline__ EpiPre epi_prefetch(const Epilogue& ep, int row_base, int col, int M, int N) {
  EpiPre p;
  const int cc = col < N ? col : N - 1;
  p.bias = ep.bias != nullptr ? ep.bias[cc] : 0.f;
  p.sc = ep.scale != nullptr ? ep.scale[cc] : 1.f;
  p.sh = ep.scale != nullptr ? ep.shift[cc] : 0.f;
  const int my_row = row_base + l31_of_lane();
  p.segv = (ep.seg != nullptr && my_row < M) ? ep.seg[my_row] : -1;
  return p;
}

// Fused per-proposal max pooling of one 32x32 sub-tile (bias already added to acc): rows of a proposal are
// consecutive -> run-length max over this lane's 16 rows, one integer atomicMax per run (values are post-ReLU,
// i.e. >= 0, so int order == float order; exact and order-independent).  The 32 segment ids of the tile come from
// ONE coalesced load (pre.segv: lane l31 <- row row_base+l31, -1 beyond M) distributed by cross-lane reads; 16
// dependent per-row loads cost more than the tile's MFMAs.
// sgs[r] = segment id of this lane's r-th row (-1 beyond M), from the tile's coalesced id vector
__device__ __forceinline__ void yl_tile_segs(int segv, int lhi, int sgs[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) sgs[r] = __shfl(segv, (r & 3) + 8 * (r >> 2) + 4 * lhi);   // all lanes active here
}
__device__ __forceinline__ void wave_epilogue_segmax(const f32x16& acc, int col, const Epilogue& ep, int N, float sc,
                                                     float sh, const int sgs[16]) {
  const bool col_ok = col < N;
  int cur_seg = -1;
  float cur = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int sg = sgs[r];
    const float v = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    if (sg != cur_seg) {
      if (cur_seg >= 0 && col_ok && cur > 0.f)
        atomicMax(reinterpret_cast<int*>(ep.pool + (long)cur_seg * ep.ldpool + col), __float_as_int(cur));
      cur_seg = sg;
      cur = v;
    } else {
      cur = fmaxf(cur, v);
    }
  }
  if (cur_seg >= 0 && col_ok && cur > 0.f)
    atomicMax(reinterpret_cast<int*>(ep.pool + (long)cur_seg * ep.ldpool + col), __float_as_int(cur));
}

// stage (optional): this wave's private [32][YL_STAGE_LD] fp32 region of LDS (free once the K loop's last barrier has
// passed).  The plain stores of a full 32 x 32 sub-tile then go row-major through it: every lane writes 16 bytes, one
// instruction covers 8 rows x 128 bytes (fp32) — instead of 4 bytes per lane and 2 rows x 128 bytes per instruction in
// the accumulator layout, 4x the store instructions for the same bytes.
constexpr int YL_STAGE_LD = 36;
__device__ __forceinline__ bool yl_stage_ok(const Epilogue& ep, int row_base, int col_base, int M, int N) {
  if (row_base + 32 > M || col_base + 32 > N) return false;
  if (ep.Yh != nullptr) return ep.ldy % 8 == 0 && (((uintptr_t)ep.Yh) & 15) == 0;
  return ep.ldy % 4 == 0 && (((uintptr_t)ep.Y) & 15) == 0;
}
// the staged sub-tile out of the wave's region as 16-byte row pieces: bf16 (two stores per lane) / fp32 (four)
__device__ __forceinline__ void yl_stage_store_bf16(const float* stage, const Epilogue& ep, int row_base, int col_base,
                                                    int lane) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int chunk = lane + 64 * t, R = chunk >> 2, c = (chunk & 3) * 8;
    const float4 x0 = *reinterpret_cast<const float4*>(stage + R * YL_STAGE_LD + c);
    const float4 x1 = *reinterpret_cast<const float4*>(stage + R * YL_STAGE_LD + c + 4);
    uint4 o;
    o.x = yl_pack_bf16(x0.x, x0.y); o.y = yl_pack_bf16(x0.z, x0.w);
    o.z = yl_pack_bf16(x1.x, x1.y); o.w = yl_pack_bf16(x1.z, x1.w);
    *reinterpret_cast<uint4*>(ep.Yh + (long)(row_base + R) * ep.ldy + col_base + c) = o;
  }
}
__device__ __forceinline__ void yl_stage_store_f32(const float* stage, const Epilogue& ep, int row_base, int col_base,
                                                   int lane) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int chunk = lane + 64 * t, R = chunk >> 3, c = (chunk & 7) * 4;
    *reinterpret_cast<float4*>(ep.Y + (long)(row_base + R) * ep.ldy + col_base + c) =
        *reinterpret_cast<const float4*>(stage + R * YL_STAGE_LD + c);
  }
}
__device__ __forceinline__ void wave_epilogue(f32x16 acc, int row_base, int col, int lhi,
                                              const Epilogue& ep, int M, int N, const EpiPre& pre,
                                              float* stage = nullptr) {
  const bool col_ok = col < N;
  const int cc = col_ok ? col : N - 1;
  if (ep.bias != nullptr) {
    const float bv = pre.bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += bv;
  }
  if (ep.stats != nullptr) {
    int cnt = M - row_base;
    cnt = cnt > 32 ? 32 : cnt;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      s += (row < M) ? acc[r] : 0.f;
    }
    s += __shfl_xor(s, 32);
    const float mu = cnt > 0 ? s / (float)cnt : 0.f;
    float m2 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float d = acc[r] - mu;
      m2 += (row < M) ? d * d : 0.f;
    }
    m2 += __shfl_xor(m2, 32);
    if (lhi == 0 && col_ok && cnt > 0) {
      float2* dst = reinterpret_cast<float2*>(ep.stats) + (long)(row_base >> 5) * N + col;
      *dst = make_float2(s, m2);
    }
  }
  const float sc = pre.sc, sh = pre.sh;
  const float floor = ep.relu ? 0.f : -INFINITY;
  if (ep.key64 != nullptr) {
    const int segv = pre.segv;
    int sgs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sgs[r] = __shfl(segv, (r & 3) + 8 * (r >> 2) + 4 * lhi);
    const bool neg = sc < 0.f;
    int cur_seg = -1;
    unsigned long long cur = 0ull;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const int sg = sgs[r];
      const float z = neg ? -acc[r] : acc[r];
      unsigned int u = __float_as_uint(z);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // order-preserving float -> uint
      const unsigned long long key = ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)row);
      if (sg != cur_seg) {
        if (cur_seg >= 0 && col_ok) atomicMax(ep.key64 + (long)cur_seg * ep.ldpool + col, cur);
        cur_seg = sg;
        cur = key;
      } else {
        cur = key > cur ? key : cur;
      }
    }
    if (cur_seg >= 0 && col_ok) atomicMax(ep.key64 + (long)cur_seg * ep.ldpool + col, cur);
    return;
  }
  if (ep.seg != nullptr) {
    int sgs[16];
    yl_tile_segs(pre.segv, lhi, sgs);
    wave_epilogue_segmax(acc, col, ep, N, pre.sc, pre.sh, sgs);
    return;
  }
  if (ep.Yh != nullptr && stage != nullptr && yl_stage_ok(ep, row_base, col - (int)(threadIdx.x & 31), M, N)) {
    const int l31s = threadIdx.x & 31, lane = threadIdx.x & 63, col_base = col - l31s;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      stage[((r & 3) + 8 * (r >> 2) + 4 * lhi) * YL_STAGE_LD + l31s] = fmaxf(fmaf(acc[r], sc, sh), floor);
    yl_stage_store_bf16(stage, ep, row_base, col_base, lane);
    return;
  }
  if (ep.Yh != nullptr) {
    // lanes l and l^1 hold neighbouring columns: each pair exchanges one value per two rows so that every lane
    // stores one packed 4-byte (col, col+1) pair for 8 of its 16 rows (even lanes: even r, odd lanes: odd r)
    const bool odd = (threadIdx.x & 1) != 0;
    const bool pair_ok = (col | 1) < N;          // both columns of the pair inside N (col < N is implied)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const float v0 = fmaxf(fmaf(acc[r], sc, sh), floor), v1 = fmaxf(fmaf(acc[r + 1], sc, sh), floor);
      const float got = __shfl_xor(odd ? v0 : v1, 1);
      const int row = row_base + ((r + (odd ? 1 : 0)) & 3) + 8 * (r >> 2) + 4 * lhi;
      const float lo = odd ? got : v0, hi = odd ? v1 : got;
      unsigned short* dst = ep.Yh + (long)row * ep.ldy + (col & ~1);
      if (row < M) {
        if (pair_ok) *reinterpret_cast<unsigned*>(dst) = yl_pack_bf16(lo, hi);
        else if (!odd && col_ok) *dst = (unsigned short)(yl_pack_bf16(lo, 0.f) & 0xFFFFu);
      }
    }
    // when N is odd the last column's even-lane owner also has to store the rows its odd partner would have
    if (!pair_ok && !odd && col_ok) {
#pragma unroll
      for (int r = 1; r < 16; r += 2) {
        const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        const float v = fmaxf(fmaf(acc[r], sc, sh), floor);
        if (row < M) ep.Yh[(long)row * ep.ldy + col] = (unsigned short)(yl_pack_bf16(v, 0.f) & 0xFFFFu);
      }
    }
    return;
  }
  float old[16];
  if (ep.agg != nullptr) {
    // CSR range boundaries of the tile's 32 rows: two coalesced loads + cross-lane reads
    const int n_l = yl_min(row_base + l31_of_lane(), M);
    const int rp_lo = ep.agg_ptr[n_l], rp_hi = ep.agg_ptr[yl_min(n_l + 1, M)];
    int q0s[16], q1s[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int off = (r & 3) + 8 * (r >> 2) + 4 * lhi;
      q0s[r] = __shfl(rp_lo, off);
      q1s[r] = __shfl(rp_hi, off);
    }
    const float* hp = ep.agg + cc;
    const int qmax = ep.agg_rows - 1;
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += 4) {      // 4 rows x 4 edges = 16 independent (clamped) loads in flight
      float v[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[j][e] = hp[(long)yl_min(q0s[r0 + j] + e, qmax) * ep.ldagg];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q0 = q0s[r0 + j], q1 = q1s[r0 + j], deg = q1 - q0;
        float sacc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) sacc += (e < deg) ? v[j][e] : 0.f;
        for (int q = q0 + 4; q < q1; ++q) sacc += hp[(long)q * ep.ldagg];
        old[r0 + j] = yl_mul_rn(sacc, 1.f / (float)(deg > 1 ? deg : 1));
      }
    }
  } else if (ep.accumulate) {   // all 16 reads issued back to back (clamped rows), one wait
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = yl_min(row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi, M - 1);
      old[r] = ep.Y[(long)row * ep.ldy + cc];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) old[r] = 0.f;
  }
  if (stage != nullptr && yl_stage_ok(ep, row_base, col - (int)(threadIdx.x & 31), M, N)) {
    const int l31s = threadIdx.x & 31, lane = threadIdx.x & 63, col_base = col - l31s;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      stage[((r & 3) + 8 * (r >> 2) + 4 * lhi) * YL_STAGE_LD + l31s] = fmaxf(fmaf(acc[r], sc, sh), floor) + old[r];
    yl_stage_store_f32(stage, ep, row_base, col_base, lane);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row_base + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    const float v = fmaxf(fmaf(acc[r], sc, sh), floor) + old[r];
    if (col_ok && row < M) ep.Y[(long)row * ep.ldy + col] = v;
  }
}
