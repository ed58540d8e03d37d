// fusion_f16x3.hip — the eval fusion pair launch (fusion_x6.hip) with the GEMM emulated by THREE half-precision products
// instead of six bfloat16 ones (f16x3.hpp), the eval forward's default: the same launch — 256 rows per 512-thread workgroup
// at K = 128 (128 per 256 at K = 64), A split once per wave into registers, W tiles double-buffered in LDS, one barrier per
// column tile, fx_plan's grid, the XCD mapping, the rider and the fx_segmax2_off / fx_segmax2_off_act
// epilogues of k_fusion_rows_x6 — with half the matrix work:
//   * per k step 6 MFMAs (v_mfma_f32_32x32x16_f16, the bf16 form's cycle count) on 4 B fragments, where x6 issues 12 on 6:
//     48 instead of 96 per wave and column tile at K = 128; one accumulator per column block, small terms first, so the
//     summation order is fixed;
//   * the W tile is 2 x 64 columns x K halves = 32 KB (x6: 48 KB): a third less L2 -> LDS traffic and LDS writes, and
//     69.6 KB of LDS for the two buffers (x6: 104 KB) — at K = 128 exactly the size of the prologue's transposition tiles;
//   * A's fragments are 2 x K/16 x 4 = 64 registers at K = 128 (x6: 96).
// Scaling.  Every row of A is multiplied by 2^s_row before the split (f16x3.hpp; the row maximum is one 64-element max chain
// per lane and one exchange with the partner lane l31 + 32 that holds the row's other k halves), every row of W — an output
// column — by 2^s_col in yolat_split_f16x2.  The accumulators start at ZERO and the epilogue un-scales each element with
// ldexp(acc, -(s_row + s_col)) before it adds the shift: exact, three vector instructions per element (integer add, v_ldexp,
// add).  The alternative — the shift pre-scaled per (row, column) as the accumulators' start value and one ldexp at the end —
// costs the same integer add and TWO ldexp per element, so the zero start is the cheaper one.  The 16 row exponents of a
// lane's accumulator rows live in 16 registers for the whole column walk (one __shfl each, once per workgroup, as the
// proposal offsets do): the epilogue needs no LDS round trip for them.
#include "x6.hpp"
#include "f16x3.hpp"
#include "fx_rows.hpp"
#include "segmax.hpp"

// One GEMM problem of the launch — only what the eval pair needs (FxProb, fusion_x6.hip, has the training and node-side
// uses' fields as well).
struct FhProb {
  const float* A; long lda; int N;
  const _Float16 *Wh, *Wl;      // yolat_split_f16x2 of the (scaled) weights [F, KD]
  const int* wexp;              // its scale exponent per weight row
  const float* tfold;
  const int* seg;               // != NULL: pooling epilogue into `out`; NULL: plain store of act(.) into out [N, ldo]
  float* out; long ldo;
  int F;
  int tm, groups, ng;
  int full = 0;
};
template <int KD, bool RIDER = false, int ACT = 0>
__global__ void __launch_bounds__(FxShape<KD>::T, 2) k_fusion_rows_f16x3(FhProb p0, FhProb p1, PoolRider rider,
                                                                         FxSlopes<ACT> slopes) {
  constexpr int T = FxShape<KD>::T, NWAVE = T / 64;
  constexpr int KS = KD / 16, RS = KD + 8, CPR = KD / 8;    // k steps, LDS row stride (halves), 16-byte chunks per row
  constexpr int CHUNKS = 2 * 64 * CPR, NW = CHUNKS / T;     // 16-byte chunks of one W tile, per thread
  static_assert(CHUNKS % T == 0, "W tile / thread mismatch");
  constexpr int TK = 64, TS = TK + 4;                       // the prologue's transposition tile: [32 rows][TK + 4] floats per wave
  constexpr int SMEM_W = 2 * 2 * 64 * RS * 2, SMEM_T = NWAVE * 32 * TS * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM_W > SMEM_T ? SMEM_W : SMEM_T];
  _Float16 (*Ws)[2 * 64 * RS] = reinterpret_cast<_Float16 (*)[2 * 64 * RS]>(smem);
  const int tid = threadIdx.x;
#include "fx_wg_map.inc"
  const float* __restrict__ A = small ? p1.A : p0.A;
  const long lda = small ? p1.lda : p0.lda;
  const int N = small ? p1.N : p0.N;
  const float* const tfold = small ? p1.tfold : p0.tfold;
  const int* const wexp = small ? p1.wexp : p0.wexp;
  const int* const seg = small ? p1.seg : p0.seg;
  float* const out = small ? p1.out : p0.out;
  const long ldo = small ? p1.ldo : p0.ldo;
  const int F = small ? p1.F : p0.F;
  const int groups = small ? p1.groups : p0.groups, ng = small ? p1.ng : p0.ng;
  const int tn = (F + 63) >> 6;
  float slope = 0.f;
  if constexpr (ACT != 0) slope = *(small ? slopes.s1 : slopes.s0);
  const int rt = whole ? logical : (small ? 0 : p0.full) + logical / groups;
  const int cg = whole ? 0 : logical % groups;
  const int ct0 = cg * ng;
  const int ngl = whole ? tn : yl_min(ng, tn - ct0);
  if (ngl <= 0) return;

  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt * (T / 2) + wave * 32;
  // everything the tile loop needs besides A goes out first: its latency runs under the A prologue
  const int sv_pre = (seg != nullptr && row0 + l31 < N) ? seg[row0 + l31] : -1;
  const _Float16* const wparts[2] = {small ? p1.Wh : p0.Wh, small ? p1.Wl : p0.Wl};
#define FX_W_CLAMP 1
#include "fx_w_movers.inc"
#undef FX_W_CLAMP
  fx_u32x4 rw[NW];
  load_w(ct0, rw);
  // shifts and column exponents of the first tile; later tiles: fetched one tile ahead, before that tile's W loads
  float t0 = tfold[yl_min(ct0 * 64 + l31, F - 1)], t1 = tfold[yl_min(ct0 * 64 + 32 + l31, F - 1)];
  int e0 = wexp[yl_min(ct0 * 64 + l31, F - 1)], e1 = wexp[yl_min(ct0 * 64 + 32 + l31, F - 1)];
  // ---- this wave's 32 rows of A: loaded row by row and turned into the MFMA operand order (lane = row, 8 consecutive k)
  // through a [32][TK + 4] fp32 tile in LDS (the weights' buffers, not yet in use), as k_fusion_rows_x6 does — but kept as
  // fp32 until the row's maximum is known: a lane holds 64 of its row's 128 values (K = 128), its partner the others
  fh_f16x8 Ah[KS], Al[KS];
  int nrow;                                                 // -(scale exponent) of row l31 of this wave
  {
    float xs[KS][8];
    float* Tt = reinterpret_cast<float*>(smem) + wave * (32 * TS);
    const int lr = lane >> 4, lc = (lane & 15) * 4;
#pragma unroll
    for (int q = 0; q < KD / TK; ++q) {
      float4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        v[i] = *reinterpret_cast<const float4*>(A + (long)yl_min(row0 + 4 * i + lr, N - 1) * lda + TK * q + lc);
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<float4*>(Tt + (4 * i + lr) * TS + lc) = v[i];
#pragma unroll
      for (int u = 0; u < TK / 16; ++u) {
        const int ks = (TK / 16) * q + u;
        const float4 a0 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi);
        const float4 a1 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi + 4);
        xs[ks][0] = a0.x; xs[ks][1] = a0.y; xs[ks][2] = a0.z; xs[ks][3] = a0.w;
        xs[ks][4] = a1.x; xs[ks][5] = a1.y; xs[ks][6] = a1.z; xs[ks][7] = a1.w;
      }
    }
    float mx = 0.f;                                         // (fmaxf drops a NaN: the maximum of the row's numbers)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(xs[ks][e]));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const int s = fh_scale_exp(mx);
    const float sc = fh_pow2(s);
    nrow = -s;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = xs[ks][e] * sc;
      fh_split8(y, Ah[ks], Al[ks]);
    }
  }
  const bool pooling = seg != nullptr;
  FxRuns runs;
  unsigned roff[16];                                    // element offset of each of the lane's rows' proposal in the output
  fx_seg_runs_off(sv_pre, lhi, (unsigned)ldo, runs, roff);
  int nr[16];                                           // -(scale exponent) of each of the lane's 16 accumulator rows
#pragma unroll
  for (int r = 0; r < 16; ++r) nr[r] = __shfl(nrow, (r & 3) + 8 * (r >> 2) + 4 * lhi);
  __syncthreads();                                          // every wave is done with its transposition tile
  store_w(0, rw);
  __syncthreads();
  for (int j = 0; j < ngl; ++j) {
    const int ct = ct0 + j, buf = j & 1;
    const int c0 = ct * 64 + l31, c1 = c0 + 32;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const float s0 = t0, s1 = t1;
    const int n0 = -e0, n1c = -e1;
    if (j + 1 < ngl) {
      t0 = tfold[yl_min(c0 + 64, F - 1)];
      t1 = tfold[yl_min(c1 + 64, F - 1)];
      e0 = wexp[yl_min(c0 + 64, F - 1)];
      e1 = wexp[yl_min(c1 + 64, F - 1)];
      load_w(ct + 1, rw);                              // in flight while the MFMAs below run
    }
    const _Float16* wb = &Ws[buf][l31 * RS + 8 * lhi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fh_f16x8 bf[4];                                  // [0] b0h [1] b1h [2] b0l [3] b1l
#pragma unroll
      for (int q = 0; q < 4; ++q) bf[q] = *reinterpret_cast<const fh_f16x8*>(wb + q * 32 * RS + 16 * ks);
      // small terms first; the empty asm pins the MFMAs' program order (k_fusion_rows_x6)
#define FH_MFMA(acc, a, b)                                          \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0); \
  asm volatile("" : "+v"(acc0), "+v"(acc1))
      FH_MFMA(acc0, Al[ks], bf[0]);
      FH_MFMA(acc1, Al[ks], bf[1]);
      FH_MFMA(acc0, Ah[ks], bf[2]);
      FH_MFMA(acc1, Ah[ks], bf[3]);
      FH_MFMA(acc0, Ah[ks], bf[0]);
      FH_MFMA(acc1, Ah[ks], bf[1]);
#undef FH_MFMA
    }
    // next W tile into the other buffer (its readers finished before the last barrier) BEFORE the epilogue, and everything
    // in flight waited for here, a whole MFMA phase after its issue (k_fusion_rows_x6)
    if (j + 1 < ngl) store_w(buf ^ 1, rw);
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
    // un-scale, then the shift: y = acc * 2^-(s_row + s_col) + t
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = ldexpf(acc0[r], nr[r] + n0) + s0;
      acc1[r] = ldexpf(acc1[r], nr[r] + n1c) + s1;
    }
    if (pooling) {
      if constexpr (ACT != 0) fx_segmax2_off_act(acc0, acc1, out, roff, (unsigned)c0, c0 < F, c1 < F, runs, slope);
      else fx_segmax2_off(acc0, acc1, out, roff, (unsigned)c0, c0 < F, c1 < F, runs);
    } else {
      // plain store of act(.) (fusion_block_super: P rows): the accumulator layout as it is — a few row tiles per launch
      unsigned rb = (unsigned)(row0 + 4 * lhi);
      asm volatile("" : "+v"(rb));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned row = rb + (r & 3) + 8 * (r >> 2);
        if ((int)row < N) {
          float* o = out + (unsigned long)row * (unsigned long)ldo;
          if constexpr (ACT != 0) {
            if (c0 < F) o[c0] = acc0[r] > 0.f ? acc0[r] : slope * acc0[r];
            if (c1 < F) o[c1] = acc1[r] > 0.f ? acc1[r] : slope * acc1[r];
          } else {
            if (c0 < F) o[c0] = fmaxf(acc0[r], 0.f);
            if (c1 < F) o[c1] = fmaxf(acc1[r], 0.f);
          }
        }
      }
    }
    __syncthreads();
  }
}

// W [rows, cols] fp32 (optionally scaled per row) -> two half-precision matrices hi / lo [rows, cols] and one scale
// exponent per row (f16x3.hpp): hi + lo == fl(row_scale * W) * 2^exp[r] to 2^-23 relative for every element within 2^16 of
// its row's largest magnitude.  One wave per row.
static __global__ void __launch_bounds__(64) k_split_f16x2(const float* __restrict__ W, long ldw, int cols,
                                                           const float* __restrict__ row_scale, _Float16* __restrict__ hi,
                                                           _Float16* __restrict__ lo, int* __restrict__ exps) {
  const long r = blockIdx.x;
  const int lane = threadIdx.x;
  const float rs = row_scale != nullptr ? row_scale[r] : 1.f;
  float mx = 0.f;
  for (int c = lane; c < cols; c += 64) mx = fmaxf(mx, fabsf(W[r * ldw + c] * rs));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  const int s = fh_scale_exp(mx);
  const float sc = fh_pow2(s);
  if (lane == 0) exps[r] = s;
  for (int c = lane; c < cols; c += 64) {
    const float x = (W[r * ldw + c] * rs) * sc;
    const _Float16 h = (_Float16)x;
    hi[r * cols + c] = h;
    lo[r * cols + c] = (_Float16)(x - (float)h);
  }
}

extern "C" int yolat_split_f16x2(const float* W, int64_t ldw, int64_t rows, int64_t cols, const float* row_scale,
                                 uint16_t* hi, uint16_t* lo, int32_t* exps, yolat_stream_t stream) {
  if (rows <= 0 || cols <= 0 || !W || !hi || !lo || !exps || ldw < cols) return YOLAT_E_INVALID;
  if (rows >= (1LL << 31) || cols >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_split_f16x2, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, W, (long)ldw, (int)cols,
                     row_scale, reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo), exps);
  YL_LAUNCH_CHECK();
  return 0;
}

namespace {
struct FxF16x3 {
  using Prob = FhProb;
  template <int KD, bool RIDER, int ACT>
  static void launch(unsigned grid, hipStream_t st, const FhProb& p0, const FhProb& p1, const PoolRider& pr, FxSlopes<ACT> sl) {
    hipLaunchKernelGGL((k_fusion_rows_f16x3<KD, RIDER, ACT>), dim3(grid), dim3(FxShape<KD>::T), 0, st, p0, p1, pr, sl);
  }
};
}  // namespace

// yl_fusion_pair_eval_x6_impl with the weights as yolat_split_f16x2 gives them (hi, lo, exponents): same contract, same
// grid, k_fusion_rows_f16x3.
int yl_fusion_pair_eval_f16x3_impl(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh, const uint16_t* Wl,
                                   const int32_t* Wexp, const float* tfold, int64_t F, const int32_t* node_seg, float* pool,
                                   int64_t ldpool, const float* S, int64_t lds, int64_t P, const uint16_t* Wsh,
                                   const uint16_t* Wsl, const int32_t* Wsexp, const float* tsfold, float* Ys, int64_t ldys,
                                   const PoolRider* rider, yolat_stream_t stream, const float* slope_f,
                                   const float* slope_s) {
  FxPairGrid g;
  YL_TRY(yl_fx_pair_setup(A, lda, N, D, tfold, F, node_seg, pool, ldpool, S, lds, P, tsfold, Ys, ldys,
                          !Wh || !Wl || !Wexp || !Wsh || !Wsl || !Wsexp,
                          !yl_aligned16(Wh) || !yl_aligned16(Wl) || !yl_aligned16(Wsh) || !yl_aligned16(Wsl),
                          /*ys_span32=*/true, rider, slope_f, slope_s, &g));
  // (leaky activation: `pool` holds -inf / 0 per proposal, yolat_pool_init_signed, not zeros)
  FhProb p0, p1;
  p0.A = A; p0.lda = lda; p0.N = (int)N; p0.Wh = reinterpret_cast<const _Float16*>(Wh);
  p0.Wl = reinterpret_cast<const _Float16*>(Wl); p0.wexp = Wexp; p0.tfold = tfold; p0.seg = node_seg; p0.out = pool;
  p0.ldo = ldpool; p0.F = (int)F;
  p0.tm = g.tm0; p0.full = g.full; p0.groups = g.groups; p0.ng = g.ng;
  p1.A = S; p1.lda = lds; p1.N = (int)P; p1.Wh = reinterpret_cast<const _Float16*>(Wsh);
  p1.Wl = reinterpret_cast<const _Float16*>(Wsl); p1.wexp = Wsexp; p1.tfold = tsfold; p1.seg = nullptr; p1.out = Ys;
  p1.ldo = ldys; p1.F = (int)F;
  p1.tm = g.tm1; p1.groups = g.tn; p1.ng = 1;
  fx_launch_rows<FxF16x3>(D, g.total, p0, p1, g.rider, slope_f, slope_s, (hipStream_t)stream);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_fusion_pair_eval_f16x3(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh,
                                            const uint16_t* Wl, const int32_t* Wexp, const float* tfold, int64_t F,
                                            const int32_t* node_seg, float* pool, int64_t ldpool, const float* S,
                                            int64_t lds, int64_t P, const uint16_t* Wsh, const uint16_t* Wsl,
                                            const int32_t* Wsexp, const float* tsfold, float* Ys, int64_t ldys,
                                            yolat_stream_t stream) {
  return yl_fusion_pair_eval_f16x3_impl(A, lda, N, D, Wh, Wl, Wexp, tfold, F, node_seg, pool, ldpool, S, lds, P, Wsh, Wsl,
                                        Wsexp, tsfold, Ys, ldys, nullptr, stream, nullptr, nullptr);
}

// the activation-aware form (yolat_fusion_pair_eval_x6_act's contract): signed start values of `pool`, then the ACT
// instantiation
extern "C" int yolat_fusion_pair_eval_f16x3_act(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh,
                                                const uint16_t* Wl, const int32_t* Wexp, const float* tfold, int64_t F,
                                                const float* slope_f, const int32_t* node_seg, const int32_t* seg_ptr,
                                                float* pool, int64_t ldpool, const float* S, int64_t lds, int64_t P,
                                                const uint16_t* Wsh, const uint16_t* Wsl, const int32_t* Wsexp,
                                                const float* tsfold, const float* slope_s, float* Ys, int64_t ldys,
                                                yolat_stream_t stream) {
  if (!slope_f || !slope_s || !seg_ptr) return YOLAT_E_INVALID;
  YL_TRY(yolat_pool_init_signed(seg_ptr, P, F, pool, ldpool, stream));
  return yl_fusion_pair_eval_f16x3_impl(A, lda, N, D, Wh, Wl, Wexp, tfold, F, node_seg, pool, ldpool, S, lds, P, Wsh, Wsl,
                                        Wsexp, tsfold, Ys, ldys, nullptr, stream, slope_f, slope_s);
}
