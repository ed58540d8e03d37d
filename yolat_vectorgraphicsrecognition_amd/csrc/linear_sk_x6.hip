// linear_sk_x6.hip — the skinny split-K Linear (few rows x long K: classifier 1 of the eval forward, P x 2304 -> 512) with
// its fp32 operand tiles brought in by LDS-DMA, as k_gemm_nt_sk_dma<8> (gemm_sk.hpp), and the products on the bf16 matrix
// cores as a bf16x6-emulated fp32 GEMM (x6.hpp) instead of the fp32-input MFMA.
// Entry point: yolat_linear_sk_x6.
//
// Why.  k_gemm_nt_sk_dma<8> spends 1024 of the 1310 cycles of a 128-deep chunk in 8 x v_mfma_f32_32x32x2_f32 x 64 cycles per
// wave, two waves per SIMD: the slowest pipe of the part, which also executes on the SIMD's vector ALUs (DESIGN.md "fp32
// MFMA and the vector ALU").  Here the bytes moved are the same (fp32 A and W, the same global_load_lds_dwordx4 pieces), a
// wave splits the 16 k it owns of each operand row in registers (fx_split8: ~36 vector instructions per 8 floats) and
// issues 6 x v_mfma_f32_32x32x16_bf16 (32 cycles each): 384 matrix-pipe cycles per SIMD and chunk instead of 1024, beside
// ~80 vector instructions x 4 cycles x 2 waves = ~640 vector-ALU cycles, which is the new limiter.
//
// Fragment reads, bank conflicts on paper.  LDS[row r][granule g'] = X[r][k0 + 4 (g' ^ (r & 15))] as in the parent.  Wave w,
// lane (l31, lhi) reads the logical granules 4 w + 2 lhi and 4 w + 2 lhi + 1 of row l31 (k = 16 w + 8 lhi .. + 7: the A / B
// operand of the 32x32x16 MFMA) at positions g ^ (l31 & 15).  A ds_read_b128 is served in four 16-lane groups, each inside
// one 32-lane half ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32): a group has one g and all 16 values of
// l31 & 15, so its 16 positions differ in their low four bits = 16 different 16-byte slots of the 256-byte bank row.  Rows
// are 512 bytes = two bank rows apart, which adds nothing.  No conflict; 4 ds_read_b128 per wave and chunk instead of 8.
//
// Results: different summation grouping than the fp32 MFMA kernels (16 k per MFMA, three partial products per (i, j) pair
// dropped at O(2^-24) relative), deterministic: fixed product order, fixed-order 8-wave reduction.  Inf / NaN as x6.hpp says.
#include "x6.hpp"
#include "operands.hpp"
#include "epilogue.hpp"
#include "gemm_nt_two.hpp"   // not launched here: see the header
#include "gemm_sk.hpp"
#include "internal.hpp"

__global__ void __launch_bounds__(512) k_gemm_nt_sk_x6dma(const float* __restrict__ A, long lda, int rowsA,
                                                         const float* __restrict__ B, long ldb, int rowsB, Epilogue ep,
                                                         int M, int N, int K, long long* stamps) {
  constexpr int NW = 8, BT = 32, BK = 128, NP = 32 / NW;            // waves, tile edge, chunk depth, DMA pieces per wave and chunk
  __shared__ __attribute__((aligned(16))) float smem[2][2][BT * BK];        // [stage][A | B][row][128]: 64 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  int rt_, ct_;
  yl_xcd_tile(rt_, ct_);
  const int row0 = rt_ * BT, col0 = ct_ * BT;
  const EpiPre pre = epi_prefetch(ep, row0, col0 + l31, M, N);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const unsigned lds0 = (unsigned)(size_t)&smem[0][0][0];
  // this wave's pieces of a stage: piece i = NP wave + j -> operand i >> 4, row pair i & 15; lane -> (row, granule)
  const float* src[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = NP * wave + j, op = i >> 4, pair = i & 15;
    const int r = 2 * pair + (lane >> 5), g = (lane & 31) ^ (r & 15);
    src[j] = op == 0 ? A + (long)yl_min(row0 + r, rowsA - 1) * lda + 4 * g : B + (long)yl_min(col0 + r, rowsB - 1) * ldb + 4 * g;
  }
  auto stage = [&](int s, int k0) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = NP * wave + j, op = i >> 4, pair = i & 15;
      yl_glds16(src[j] + k0, lds0 + (unsigned)(((s * 2 + op) * BT * BK + pair * 256) * 4));
    }
  };
  // this lane's two granules of a row: k = 16 wave + 8 lhi .. + 7 of the chunk
  const int g0 = 4 * wave + 2 * lhi;
  const int off0 = l31 * BK + 4 * (g0 ^ (l31 & 15)), off1 = l31 * BK + 4 * ((g0 + 1) ^ (l31 & 15));
  auto compute = [&](int s) {
    const float* As = &smem[s][0][0];
    const float* Bs = &smem[s][1][0];
    const float4 a0 = *reinterpret_cast<const float4*>(As + off0), a1 = *reinterpret_cast<const float4*>(As + off1);
    const float4 b0 = *reinterpret_cast<const float4*>(Bs + off0), b1 = *reinterpret_cast<const float4*>(Bs + off1);
    const float a8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float b8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    fx_bf16x8 ah, am, al, bh, bm, bl;
    fx_split8(a8, ah, am, al);
    fx_split8(b8, bh, bm, bl);
    // small terms first (fusion_x6.hip's order); one accumulator: the chain of dependences is the summation order
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  };
  const int nch = K / BK;
  long long t0 = 0, t_wait = 0, t_comp = 0;
  const bool st_on = stamps != nullptr && tid == 0;
  stage(0, 0);
  for (int kc = 0; kc < nch; ++kc) {
    long long ta = 0, tb = 0, tc = 0;
    if (kc + 1 < nch) {
      stage((kc + 1) & 1, (kc + 1) * BK);
      if (st_on) ta = clock64();
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                  // this chunk's pieces have landed; the next chunk's stay in flight
    } else {
      if (st_on) ta = clock64();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // every wave's pieces of the chunk are in LDS
    if (st_on) tb = clock64();
    compute(kc & 1);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the stage may be overwritten (two iterations on)
    if (st_on) { tc = clock64(); t_wait += tb - ta; t_comp += tc - tb; if (kc == 0) t0 = ta; }
  }
  if (st_on) {
    const long o = 3 * (blockIdx.x + (long)gridDim.x * blockIdx.y);
    stamps[o] = t_wait; stamps[o + 1] = t_comp; stamps[o + 2] = clock64() - t0;
  }
  // fixed-order reduction of the 8 K-partials: waves 1.. park theirs in LDS, wave 0 adds them in wave order
  float* red = &smem[0][0][0];   // [NW - 1][16][64]
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < NW - 1; ++w)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += red[(w * 16 + r) * 64 + lane];
    wave_epilogue(acc, row0, col0 + l31, lhi, ep, M, N, pre);
  }
}

static bool yl_linear_sk_x6_ok(const float* A, int64_t lda, int64_t M, int64_t K, const float* W, int64_t ldw, int64_t Nout) {
  return M > 0 && Nout > 0 && K >= 128 && K % 128 == 0 && K < (1LL << 31) && lda % 4 == 0 && ldw % 4 == 0 && yl_aligned16(A) &&
         yl_aligned16(W) && M <= 65536 && Nout <= 65536;
}

// Y [M, Nout] = epi(A [M, K] . W [Nout, K]^T + bias), epi = o_scale / o_shift (nullable pair) then ReLU (o_relu).
// K % 128 == 0, lda % 4 == 0, ldw % 4 == 0, A and W 16-byte aligned, M, Nout <= 65536: else YOLAT_E_UNSUPPORTED.
extern "C" int yolat_linear_sk_x6(const float* A, int64_t lda, int64_t M, int64_t K, const float* W, int64_t ldw,
                                  const float* bias, int64_t Nout, const float* o_scale, const float* o_shift, int o_relu,
                                  float* Y, int64_t ldy, yolat_stream_t stream) {
  if (M < 0 || K <= 0 || Nout <= 0 || (M > 0 && (!A || !Y)) || !W) return YOLAT_E_INVALID;
  if (M >= (1LL << 31) || lda < K || ldw < K || ldy < Nout) return YOLAT_E_INVALID;
  if ((o_scale == nullptr) != (o_shift == nullptr)) return YOLAT_E_INVALID;
  if (M == 0) return 0;
  if (!yl_linear_sk_x6_ok(A, lda, M, K, W, ldw, Nout)) return YOLAT_E_UNSUPPORTED;
  Epilogue ep;
  ep.bias = bias; ep.scale = o_scale; ep.shift = o_shift; ep.relu = o_relu;
  ep.Y = Y; ep.ldy = ldy; ep.accumulate = 0; ep.stats = nullptr; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  // one workgroup per 32 x 32 outputs; the 2-D grid is flattened by yl_xcd_tile (at most 2048 x 2048 tiles)
  const dim3 grid(yl_cdiv(M, 32), yl_cdiv(Nout, 32));
  hipLaunchKernelGGL(k_gemm_nt_sk_x6dma, grid, dim3(512), 0, (hipStream_t)stream, A, (long)lda, (int)M, W, (long)ldw, (int)Nout,
                     ep, (int)M, (int)Nout, (int)K, yl_gemm_sk_dma_stamps());      // stamps: tools/exp/lds_dma_bench.py only
  YL_LAUNCH_CHECK();
  return 0;
}
